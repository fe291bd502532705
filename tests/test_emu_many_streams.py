"""The schedules bench.py runs and no parity test reached, on the CPU emulation build: 4 ... 17 streams in one context, calls of 16 and
32 frames, the per-frame loop and the depth-1 pipeline at 4 streams, the production strip kernels at 5 streams -- every stream on a
clip of its own, the oracle's bytes bit for bit (tests/parity_matrix.py: MANY_*; helpers.frames_clip, helpers.pipelined_clip).  Host
logic, batch indexing and the range-checked buffer resources of the emulation; the gfx950 build runs the same cases in
tests/test_gpu_exact.py and tests/test_gpu_riesz_exact.py.

Frames that lie more than 4 GiB apart: helpers.far_clip and the far cases of the other device surfaces (parity_matrix.FAR_*)."""
import pytest

import parity_matrix as M
from helpers import HostMem, pipelined_clip

HOST = HostMem()


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


@pytest.mark.parametrize("idx,w,h,levels,ns", M.MANY_CASES, ids=_ids(M.MANY_CASES))
def test_emu_many_streams_full_batches(lvm, po, emu, idx, w, h, levels, ns):
    M.many_streams_case(lvm, po, emu, HOST, idx, w, h, levels, ns)


@pytest.mark.parametrize("idx,ns", M.MANY_PER_FRAME, ids=_ids(M.MANY_PER_FRAME))
def test_emu_many_streams_per_frame_schedule(lvm, po, emu, idx, ns):
    M.many_per_frame(lvm, po, emu, HOST, idx, ns)


@pytest.mark.parametrize("nframes,ring", M.MANY_PIPELINE, ids=_ids(M.MANY_PIPELINE))
def test_emu_four_streams_pipelined(lvm, po, emu, nframes, ring):
    pipelined_clip(lvm, po, emu, HOST, 64, 48, 3, nframes, ring=ring, n_streams=4)


# the Riesz set at 264 x 150 takes the emulation half a minute at five streams: here 136 x 78, two levels (136 and 68 wide: every strip
# kernel and the dword-wide frame I/O stay eligible, as the asserted launches show); the gfx950 run keeps the entry's size
EMU_FORCED_SIZE = {"rz_strips": (136, 78, 2)}


@pytest.mark.parametrize("force", list(M.LAYOUT_FORCED))
def test_emu_five_streams_forced_strip_kernels(lvm, po, emu, force):
    M.many_forced(lvm, po, emu, HOST, force, size=EMU_FORCED_SIZE.get(force))


@pytest.mark.parametrize("key", list(M.FAR_CASES))
def test_emu_far_surfaces(lvm, po, emu, key):
    M.far_case(lvm, po, emu, HOST, key)


@pytest.mark.parametrize("surface", list(M.FAR_SURFACES))
def test_emu_far_units_of_the_other_device_surfaces(lvm, po, emu, surface):
    M.FAR_SURFACES[surface](lvm, po, emu, HOST)
