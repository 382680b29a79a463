"""The CPU harness of the launch planner (tests/host_harness/msm_plan_harness.cpp, tests/test_msm_plan_host.py) and the library that runs agree: on
BN254, for every base mode, a single MSM, a 3-vector batch from device memory, a 2-of-16 window share (plain bases) and a sparse run (not on wide
tables) -- after each call env_report()'s shape of the last launch must be what the harness plans from the same inputs, the device's compute units
as torch reports them, and each result is the CPU oracle's."""
import numpy as np
import pytest
import torch

import msm_webgpu_amd as m
from oracle import cpu
from tests.test_msm_plan_host import OK, build, context, line, run

pytestmark = pytest.mark.gpu
SIZES = [3000, 70000]
MODES = ["plain", "endomorphism", "tables", "wide"]
REPORTED = {"last_mode": "mode", "last_wbits": "wbits", "last_w_count": "w_count", "last_chunk_len": "chunk_len", "last_chunks": "chunks", "last_planes": "planes",
            "last_list_path": "list_path", "last_identity_mask": "mask"}


@pytest.fixture(scope="module")
def inputs(built, tmp_path_factory):
    """the harness, points, three scalar vectors and the oracle's three answers per size: computed once, read by every mode"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    exe = build(tmp_path_factory.mktemp("msm_plan_gpu"), "msm_plan_harness", ["-O2"])
    data = {}
    for n in SIZES:
        points = cpu.sample_points(7300 + n, n)
        vectors = [cpu.sample_scalars(7400 + n + k, n) for k in range(3)]
        data[n] = points, vectors, [cpu.to_affine64(cpu.cpu_msm(points, v, n_threads=16)) for v in vectors]
    return exe, data


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", SIZES)
def test_the_library_runs_what_the_harness_plans(inputs, n, mode):
    exe, data = inputs
    points, vectors, want = data[n]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    c = m.MsmContext(0)
    try:
        c.set_bases(points, endomorphism=mode == "endomorphism", precompute="wide" if mode == "wide" else mode == "tables")
        ctx = context("canonical", "plain" if mode == "wide" else mode, 0, n_bases=n, cus=cus, wide_bits=c.wide_bits())  # (the width: the library's choice)
        assert (ctx["wide_bits"] != 0) == (mode == "wide") and c.uses_endomorphism() == (mode == "endomorphism")

        def agrees(what, case):
            (p,) = run(exe, [case], inherit=True)
            rep = c.env_report()
            assert p["rc"] == OK and {k: rep[k] for k in REPORTED} == {k: p[v] for k, v in REPORTED.items()}, (what, p, rep)

        dev = [torch.frombuffer(bytearray(v), dtype=torch.uint8).cuda() for v in vectors]
        # one MSM
        assert c.msm(dev[0]).to_affine_bytes() == want[0]
        agrees("single", line("plan", whole=1, n=n, sync=1, **ctx))
        # three vectors through msm_hip_run_batch_device: the report is the last group's launch
        got = c.msm_batch(torch.cat(dev), n)
        assert [g.to_affine_bytes() for g in got] == want
        (g,) = run(exe, [line("group", n=n, batch=3, **ctx)], inherit=True)
        last = 3 - g["group"] * ((3 + g["group"] - 1) // g["group"] - 1)
        agrees("batch", line("plan", whole=1, n=n, nvec=last, **ctx))
        if mode == "plain":  # the 16 windows as 8 shares of 2, each to device memory
            sums = torch.empty((16, c.jb), dtype=torch.uint8, device="cuda")
            for w in range(0, 16, 2):
                c.msm_windows(dev[1], w, w + 2, sums[w:w + 2])
                agrees("share %d" % w, line("plan", n=n, w_begin=w, w_end=w + 2, sums_dev=1, **ctx))
            assert m.MsmContext.combine_windows(sums.cpu().numpy().tobytes()).to_affine_bytes() == want[1]
        if mode != "wide":  # the same sum with its entries in another order, through the sparse call
            perm = np.random.default_rng(n).permutation(n)
            sc = np.frombuffer(vectors[2], dtype=np.uint8).reshape(n, 32)[perm]
            got = c.msm_sparse(torch.from_numpy(perm).cuda(), torch.from_numpy(np.ascontiguousarray(sc)).cuda())
            assert got.to_affine_bytes() == want[2]
            agrees("sparse", line("plan", whole=1, sparse=1, indices=1, n=n, sync=1, **ctx))
    finally:
        c.close()
