"""One context across mixed surfaces and changing caller streams.

The parity tests hold every kernel to the oracle shape by shape, and helpers.run_schedules shows that each call surface ALONE gives the
same bytes -- each in a context of its own.  Here ONE context goes through a seeded interleaving of everything a caller may do to it
(helpers.draw_plan: lvm_process, lvm_process_device, lvm_process_device_frames in 1 .. 33 frames, lvm_chain_process_batch_ex,
an lvm_export_frames segment, lvm_set_pipeline + lvm_flush, lvm_set_max_frames, amplification and cutoff changes, lvm_reset) and every
frame must be the oracle's: the temporal state -- IIR planes, Riesz filter state, Color's ring, the parity-buffered pyramids, the owed
pipelined frame, the batch arena -- is one, whatever surface touches it next.

CPU part: the emulation build, exact flavour, byte for byte.  It checks the synchronous host logic; its streams and events do nothing.

GPU part (-m gpu): the same plans with real caller streams (helpers.StreamMem).  include/lvm_hip.h promises that the calls of one context
take effect in call order on whatever streams they are given; the test does the caller's duties only (its buffers) and makes the order
impossible to get right by luck: every other call sits behind a device-side delay of 25 ms on its stream, and the call after it goes to
another stream, or to a host surface, at once.  A library that does not order its hidden state across streams reads the state from before
the previous frame and misses the oracle on the first try; nothing is repeated, nothing relies on a race window.  Laplace and Color:
exact flavour, byte for byte.  Riesz (device acosf / sinf / cosf): the parity bars against the oracle and byte identity with the same plan
run entirely on the own stream of a second context.

Without the ordering in csrc/lvm_api.hip (order_after_previous) 12 of the 17 GPU cases miss the oracle, the first at frames 1 .. 34 of
their plans with 326 .. 657 149 differing bytes.  The other five pass either way: their few stream changes fall where something else orders the calls (a host wait inside the library, as
when the state is built or lvm_process grows its staging buffers; probably also streams that the HIP runtime maps onto one hardware queue).

Not raced on purpose: before lvm_reset, before a temporal batch that makes the batch buffers grow and before lvm_destroy the plans wait for
the device (helpers.run_plan).  That those paths wait for every caller stream is read from csrc/lvm_api.hip (sync_streams) and not tried
by letting a free meet a delayed kernel.

Measured on the CPU (one core): 0.1 .. 0.3 s per Laplace case, 0.4 .. 1.4 s per Color case (40 frames), 1.9 s per Riesz case."""
import numpy as np
import pytest

from helpers import HostMem, StreamMem, TorchMem, check_plan, check_plans_identical, draw_plan, plan_frames, plan_reference, run_plan

# name: (synth.config index, w, h, levels, frames per plan, frames before the first batch, fps, parameter overrides)
SHAPES = {
    "laplace-96x64-L4": (0, 96, 64, 4, 25, 0, None, {}),
    "laplace-67x45-L3": (0, 67, 45, 3, 25, 0, None, {}),          # odd sizes and strides: the byte kernels
    "riesz-96x64-L3": (2, 96, 64, 3, 25, 0, None, {}),
    "color-64x48-L2": (3, 64, 48, 2, 40, 18, 7.0, {"coLow": 0.4, "coHigh": 2.0}),      # 7 fps: a 16-frame window, full before the first batch
}
PRODUCTION = {"laplace-640x360-L4": (0, 640, 360, 4, 0, 0, None, {})}          # GPU only: the benchmark's small shape
SEEDS = (0, 1, 2)
_CASES = {}


def _setup(lvm, shape, n_streams=1):
    idx, w, h, levels, n, warm, fps, over = {**SHAPES, **PRODUCTION}[shape]
    ck, pk = lvm.synth.config(idx, (w, h, levels))
    if fps is not None:
        ck["fps"] = fps; pk["framerate"] = fps
    pk.update(over)
    clips = [lvm.synth.Clip(seed=1234 + s, **ck) for s in range(n_streams)]
    return pk, clips, n, warm


def _plan_seed(shape, seed):
    return 10 * sorted(SHAPES).index(shape) + seed          # every shape its own plans


def _frames(clips, n):
    return np.stack([np.stack([c.frame(t) for c in clips]) for t in range(n)])          # [frame][stream][h][w][3]


def _case(lvm, po, shape, seed, n_streams=1):
    """(plan, frames, parameters, oracle result) of a drawn case: computed once, shared by the CPU and the GPU test, never written to"""
    key = (shape, seed, n_streams)
    if key not in _CASES:
        pk, clips, n, warm = _setup(lvm, shape, n_streams)
        plan = draw_plan(_plan_seed(shape, seed), n, pk["mode"], n_streams, warm, pk["framerate"])
        frames = _frames(clips, n)
        _CASES[key] = (plan, frames, pk, plan_reference(po, plan, frames, pk))
    return _CASES[key]


def _fixed_case(lvm, po, name, shape, plan, n_streams=1):
    if name not in _CASES:
        pk, clips, _, _ = _setup(lvm, shape, n_streams)
        frames = _frames(clips, plan_frames(plan))
        _CASES[name] = (plan, frames, pk, plan_reference(po, plan, frames, pk))
    return _CASES[name]


# ---- CPU: the emulation build ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_mixed_surfaces_bit_exact(lvm, po, emu, shape, seed):
    plan, frames, pk, ref = _case(lvm, po, shape, seed)
    assert any(ref[0]), "no frame produced"
    check_plan(plan, ref, run_plan(lvm, emu, HostMem(), plan, frames, pk))


def test_plans_cover_every_operation(lvm):
    """the drawn plans, taken together, hold every operation, batches up to the frames that are left, and both pipeline depths"""
    seen, longest = set(), 0
    for shape in SHAPES:
        idx, w, h, levels, n, warm, fps, _ = SHAPES[shape]
        mode = lvm.synth.config(idx, (w, h, levels))[1]["mode"]
        for seed in SEEDS:
            plan = draw_plan(_plan_seed(shape, seed), n, mode, 1, warm, fps or 30.0)
            assert plan_frames(plan) == n
            seen |= {op[0] for op in plan} | {op for op in plan if op[0] == "pipeline"}
            longest = max([longest] + [op[1] for op in plan if op[0] == "frames"])
            t = 0
            for op in plan:          # the first `warm` frames go one per call
                nf = (op[1] if len(op) > 1 else 1) if op[0] in ("host", "device", "frames", "chain", "export") else 0
                assert nf <= 1 or t >= warm, (shape, seed, op, t)
                t += nf
    assert seen >= {"host", "device", "frames", "chain", "export", "pipeline", ("pipeline", 0), ("pipeline", 1), "flush", "max_frames", "set",
                    "reset"}, seen
    assert longest >= 9, longest


# ---- GPU: the same plans on real caller streams -------------------------------------------------------------------------------------
def _gpu_check(lvm, hip, plan, frames, pk, ref, mem):
    res = run_plan(lvm, hip, mem, plan, frames, pk)
    late = [k for k, l in mem.log if l and k >= 0]
    assert late, "no call of the plan sat behind a delay"
    if pk["mode"] != 1:
        worst = check_plan(plan, ref, res)
    else:
        worst = check_plan(plan, ref, res, exact=False)                                  # (the bars of helpers.oracle_bars: 1 LSB, >= 0.999 identical)
        check_plans_identical(plan, res, run_plan(lvm, hip, TorchMem(), plan, frames, pk))          # ... and the own stream's bytes
    print("calls (stream, late):", mem.log, "worst u8 diff / identical:", worst)


@pytest.mark.gpu
def test_caller_streams_are_not_the_own_stream():
    """Every other GPU test hands the library torch.cuda.current_stream().cuda_stream.  For torch's default stream that is the null handle,
    which lvm_api.hip maps to the context's own stream: those tests never left it.  The streams of StreamMem do."""
    import torch
    assert torch.cuda.current_stream().cuda_stream == 0
    assert TorchMem().stream() == 0
    handles = StreamMem(0).handles()
    assert len(handles) == 4 and len(set(handles)) == 4 and all(handles), handles


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_mixed_surfaces_on_caller_streams(lvm, po, hip, shape, seed):
    plan, frames, pk, ref = _case(lvm, po, shape, seed)
    _gpu_check(lvm, hip, plan, frames, pk, ref, StreamMem(100 + seed))


@pytest.mark.gpu
def test_production_batches_on_caller_streams(lvm, po, hip):
    """640 x 360, 4 levels, batches of 32 frames: the kernels the benchmark times are the ones ordered.  The first lvm_process builds the
    state and the staging buffers (both wait for the streams on the host, which would order the calls around them); then a frame behind
    a delay, a batch on another stream at once, the next batch behind a delay, lvm_process at once, a short batch behind a delay and a
    frame at once."""
    plan = [("max_frames", 32), ("host",), ("device",), ("frames", 32), ("frames", 32), ("host",), ("frames", 3), ("device",)]
    plan, frames, pk, ref = _fixed_case(lvm, po, "production", "laplace-640x360-L4", plan)
    _gpu_check(lvm, hip, plan, frames, pk, ref, StreamMem(7, own=False))


@pytest.mark.gpu
def test_two_stream_context_on_caller_streams(lvm, po, hip):
    plan, frames, pk, ref = _case(lvm, po, "laplace-96x64-L4", 3, n_streams=2)
    _gpu_check(lvm, hip, plan, frames, pk, ref, StreamMem(11))


@pytest.mark.gpu
def test_flush_on_another_stream_than_the_call_it_completes(lvm, po, hip):
    """pipeline depth 1: the call that owes a frame sits behind a delay, the lvm_flush that completes it goes to another stream at once"""
    plan = [("pipeline", 1), ("device",), ("flush",), ("device",), ("device",), ("device",), ("flush",), ("device",), ("frames", 4),
            ("device",), ("flush",), ("host",), ("device",), ("flush",)]
    plan, frames, pk, ref = _fixed_case(lvm, po, "flush", "laplace-96x64-L4", plan)
    mem = StreamMem(13, own=False)
    _gpu_check(lvm, hip, plan, frames, pk, ref, mem)
    streamed = [op for op in plan if op[0] in ("device", "frames", "flush")]          # one entry of mem.log each
    flushes = [i for i, op in enumerate(streamed) if op[0] == "flush"]
    assert any(not mem.log[i][1] and mem.log[i - 1][1] and mem.log[i][0] != mem.log[i - 1][0] for i in flushes), mem.log


@pytest.mark.gpu
def test_ten_caller_streams_then_a_structural_change(lvm, po, hip):
    """Ten distinct streams in turn: more than the context keeps events for (kMaxCallerStreams = 8), so slots are recycled and the overflow
    flag is set.  The plan ends with a level change: the structural reset frees the old state behind sync_streams, which must have covered
    every one of them, and the frames behind it are the oracle's again."""
    plan = [("device",)] + [("frames", n) for n in (2, 1, 2, 1, 3, 1, 2, 1, 2, 1, 4, 1, 2, 1, 3, 1, 2, 1, 2, 1, 2)]
    plan += [("set", {"levels": 3}), ("device",), ("frames", 3)]
    plan, frames, pk, ref = _fixed_case(lvm, po, "ten-streams", "laplace-96x64-L4", plan)
    mem = StreamMem(17, n_streams=10, own=False, cycle=True)
    _gpu_check(lvm, hip, plan, frames, pk, ref, mem)
    assert len({k for k, _ in mem.log}) == 10
