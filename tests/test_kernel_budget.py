"""Register budget of the last Laplace kernel, from the compiler's own resource report (tools/kru.sh: laplace.hip compiled for gfx950
with the Makefile's flags; no GPU involved).

k_lap_final_v4 runs 512-thread workgroups, eight waves each.  A SIMD of gfx950 has 512 VGPRs per lane, handed out in blocks of 8: up to
80 VGPRs it holds six waves, from 81 on five -- and five waves per SIMD are twenty per CU, of which two workgroups use sixteen.  The
default instance (motion, no float frame, table flavour: <true, false, 0>) is therefore held at <= 80 VGPRs, WITHOUT scratch, so that three
workgroups are resident per CU (3 x its LDS must fit the CU's 160 KB as well); the launch code sizes the persistent grid from the
occupancy the runtime reports for it.  No other instance may spill either: a budget that one of them cannot meet shows up here as scratch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
LDS_PER_CU = 163840


@pytest.fixture(scope="module")
def usage():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc is not installed")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "kru.sh"), "laplace.hip"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"vgpr (\d+) sgpr (\d+) scratch (\d+) occ (\d+) lds (\d+) (?:void )?(?:lvm::)?(k_lap_final_v4<.*>)\s*$", line)
        if m:
            rows[m.group(6).replace(" ", "")] = dict(zip(("vgpr", "sgpr", "scratch", "occ", "lds"), map(int, m.groups()[:5])))
    assert len(rows) == 12, (r.returncode, sorted(rows), r.stdout[-2000:])          # MOTION x DBG x three flavours
    return rows


def test_default_last_kernel_holds_six_waves_per_simd(usage):
    u = usage["k_lap_final_v4<true,false,0>"]
    print(u)
    assert u["vgpr"] <= 80, u
    assert u["scratch"] == 0, u
    assert u["occ"] >= 6, u
    assert 3 * u["lds"] <= LDS_PER_CU, u


def test_no_last_kernel_instance_spills(usage):
    spilling = {k: u for k, u in usage.items() if u["scratch"] != 0}
    assert not spilling, spilling
