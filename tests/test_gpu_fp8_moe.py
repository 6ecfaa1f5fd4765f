"""FP8 fused-MoE expert mat-muls (`FusedMoeFp8::forward_with_routing`, layers/moe.rs:1429-1481) through `Fp8MoE`: the routed op against
the per-pair f64 product of the exactly decoded weights, the packed gate|up scale rows, ids of other ranks, a NaN weight code, the
refusals, and the captured layer.  Route of csrc/fp8_moe.hip: fewer pairs than experts: the streaming kernel (runs of <= 16 pairs);
else the GEMM (runs of <= 64)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import gptq as G                                                    # noqa: E402
from tests.test_cpu_fp8_moe import NAMES, REFUSALS, call                        # noqa: E402
from tests.test_gpu_fp8_linear import FINITE, case                              # noqa: E402
from tests.test_gpu_linear import ULP, check_ulp, cv, dev16, host16             # noqa: E402,F401
from tests.test_gpu_mxfp4_moe import pad, products, routing                     # noqa: E402


def experts(cv, E, N, K, n_half=0, poison=None, seed=0):
    """every expert by the dense test's recipe (all 254 finite codes, scales that are no powers of two) with a seed of its own; n_half:
    gate and up built apart and packed by `cat`, scales too, as the reference does (moe.rs:1385-1386).  The op object (the other
    projection is a dummy of one tile) and the f64 matrices"""
    halves = (n_half, N - n_half) if n_half else (N,)
    w, s, deq = (np.stack([np.concatenate([case(n, K, seed + N + K + 2 * e + h)[i] for h, n in enumerate(halves)]) for e in range(E)])
                 for i in range(3))
    assert np.isin(FINITE, w).all()
    if poison:
        w[poison] = 0x7F
    real = [torch.from_numpy(w).cuda(), torch.from_numpy(s).cuda()]
    dummy = [torch.zeros((E, 32, 128), dtype=torch.uint8, device="cuda"), torch.ones((E, 1 + bool(not n_half), 1), device="cuda")]
    return cv.Fp8MoE(*(real + dummy if n_half else dummy + real)), deq


def run(moe, x, ids, dt, wts=None, which="down", **kw):
    w = torch.from_numpy(wts).cuda() if wts is not None else None
    return host16(moe.gemm(dev16(x, dt), torch.from_numpy(ids).cuda(), which=which, topk_weights=w, **kw), dt)


# (counts per expert, top_k, N, K, one x row per token?, weights?); E = len(counts), the GEMM from sum(counts) >= E
CASES = [((1, 0, 1, 0), 2, 144, 384, True, True),           # decode: one token, two runs of one pair, two experts without a pair
         (pad((16,), 17), 2, 16, 128, False, False),        # all pairs on one expert: exactly one full run; one tile, one k-block
         (pad((17, 3, 0, 1), 22), 3, 144, 384, True, False),  # 17: a second run of one pair
         (pad((17, 8, 7), 33), 2, 144, 384, True, True),    # 32 pairs and 33 experts: the streaming kernel ...
         (pad((17, 8, 7), 32), 2, 144, 384, True, True),    # ... and 32: the GEMM, at the same counts
         ((64, 65), 3, 272, 384, False, True),              # GEMM: a full run | a full run and one pair; N = 272: two full scale rows and a ragged one, a ragged 128-row tile
         ((130, 6), 2, 16, 128, True, False),               # three runs, the last ragged
         # the GEMM keeps its scales in a panel staged once, so nothing of them turns over: 34 k-blocks walk the panel's row and send
         # the two operand buffers round 34 times
         ((20, 12), 2, 16, 4352, False, True),
         # 41 k-blocks for one pair: wave 0 owns six of them, so its 4-deep register ring is refilled and wraps; one staging pass of six
         ((0, 1), 1, 16, 5248, True, True)]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("counts,top_k,N,K,per_token,weighted", CASES)
def test_moe_gemm_matches_per_pair_f64_product(cv, dt, counts, top_k, N, K, per_token, weighted):
    moe, deq = experts(cv, len(counts), N, K)
    ids, wts = routing(counts, top_k)
    x_div = top_k if per_token else 1
    x = G.round_dt(np.random.default_rng(N + K).normal(0, 1, (ids.size // x_div, K)), dt)
    y = run(moe, x, ids, dt, wts if weighted else None)
    ref = G.round_dt((wts.reshape(-1, 1) if weighted else 1.0) * products(x, deq, ids, x_div), dt)
    assert np.abs(ref).max() < 65504
    print(f"{counts} N={N} K={K} {dt}: max |err| / max |ref| = {np.abs(y - ref).max() / np.abs(ref).max():.3e}")
    # both operands exact, f32 accumulation: the dense op's bound (the f32 multiply by w_p adds 2^-24 relative, inside its margin)
    check_ulp(y, ref, dt, ulps=1.01, what="fp8 moe gemm")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("counts", [pad((3, 0, 2, 1), 7), (40, 30)])             # one per kernel
def test_moe_gemm_packed_scale_rows(cv, dt, counts):
    """n_half = 144: gate uses scale rows 0 - 1, up rows 2 - 3 of `cat(gate_scale, up_scale)`; r / 128 over the packed matrix fails here"""
    N, K = 288, 384
    moe, deq = experts(cv, len(counts), N, K, n_half=N // 2)
    ids, _ = routing(counts, 2)
    x = G.round_dt(np.random.default_rng(5).normal(0, 0.05, (ids.shape[0], K)), dt)      # (gate * up stays finite in f16)
    mm = G.round_dt(products(x, deq, ids, 2), dt)
    check_ulp(run(moe, x, ids, dt, which="gate_up"), mm, dt, ulps=1.01, what="packed gate|up, stored")
    y = run(moe, x, ids, dt, which="gate_up", epilogue=cv.EPI_SILU_MUL)
    assert np.isfinite(y).all() and y.shape == (ids.size, N // 2)
    check_ulp(y, G.silu_mul16(mm[:, :N // 2], mm[:, N // 2:], dt), dt, ulps=2.01, what="silu(gate) * up", mag=mm[:, N // 2:])


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("counts", [pad((5, 3, 0, 4), 13), (30, 44)])            # one per kernel
def test_moe_gemm_ids_of_other_ranks_give_zero_rows(cv, dt, counts):
    E, N, K = len(counts), 144, 256
    moe, deq = experts(cv, E, N, K)
    ids, wts = routing(counts, 2)
    ids.reshape(-1)[[1, 6]] = -1, E
    x = G.round_dt(np.random.default_rng(9).normal(0, 1, (ids.shape[0], K)), dt)
    out = torch.full((ids.size, N), 7.0, dtype=dev16(x, dt).dtype, device="cuda")
    y = run(moe, x, ids, dt, wts, out=out)
    assert (y[[1, 6]] == 0).all()
    check_ulp(y, G.round_dt(wts.reshape(-1, 1) * products(x, deq, ids, 2), dt), dt, ulps=1.01, what="rows beside the zero rows")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("counts", [pad((2, 3, 1), 7), (20, 30, 10)])            # one per kernel
def test_moe_gemm_nan_code_poisons_its_row_for_its_expert_alone(cv, dt, counts):
    moe, deq = experts(cv, len(counts), 32, 256, poison=(1, 21, 5))
    ids, _ = routing(counts, 2)
    x = G.round_dt(np.random.default_rng(3).normal(0, 1, (ids.size, 256)), dt)
    y = run(moe, x, ids, dt)
    hit = np.zeros(y.shape, bool)
    hit[ids.reshape(-1) == 1, 21] = True
    assert (np.isnan(y) == hit).all()
    check_ulp(y[~hit], G.round_dt(products(x, deq, ids, 1), dt)[~hit], dt, ulps=1.01, what="beside the NaN row")


@pytest.mark.parametrize("what,kw", REFUSALS)
def test_moe_gemm_refuses_before_any_launch(cv, what, kw):
    from candle_vllm_amd import lib
    tdt = torch.float32 if kw.get("dtype") == 0 else torch.bfloat16
    t = {"out": torch.full((4, 64), 7.0, dtype=tdt, device="cuda"), "x": torch.ones((4, 192), dtype=tdt, device="cuda"),
         "w": torch.zeros(4 * 64 * 192, dtype=torch.uint8, device="cuda"), "s": torch.ones(16, dtype=torch.float32, device="cuda"),
         "ids": torch.zeros(4, dtype=torch.int32, device="cuda"), "wts": torch.ones(4, dtype=torch.float32, device="cuda")}
    assert set(t) == set(NAMES)
    rc = call(lib, {k: v.data_ptr() for k, v in t.items()}, **kw)
    torch.cuda.synchronize()
    assert rc != 0 and bool((t["out"] == 7.0).all()), (what, rc)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("T,counts3", [(1, ((1, 0, 1, 0), (0, 0, 1, 1), (0, 2, 0, 0))),            # one per kernel
                                       (16, ((14, 5, 6, 7), (0, 20, 0, 12), (8, 8, 15, 1)))])
def test_moe_layer_forward_captured_replays_new_routing(cv, dt, T, counts3):
    """`Fp8MoE.forward` (gate|up with SILU_MUL, down with weights, sum over top_k) in a graph: replays with other ids and weights in the
    same buffers == eager bit for bit, and within the bound composed of the two ops' bounds of the f64 layer"""
    E, top_k, H, I, XS = 4, 2, 256, 128, 0.05                   # x ~ N(0, 0.05): the layer's largest value stays far below 65504 (f16)
    gu, dn = (tuple(np.stack(a) for a in zip(*(case(n, k, 50 + n + e) for e in range(E)))) for n, k in ((2 * I, H), (H, I)))
    moe = cv.Fp8MoE(*(torch.from_numpy(a).cuda() for a in gu[:2] + dn[:2]))     # (I = 128: one scale row per half, cat == the plain rows)
    x = G.round_dt(np.random.default_rng(1).normal(0, XS, (T, H)), dt)
    xd = dev16(x, dt)
    routes = [routing(c, top_k) for c in counts3]
    ids, wts = (torch.from_numpy(a).cuda() for a in routes[0])
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        moe.forward(xd, ids, wts)                                               # warm-up: the plan's work space exists before the capture
        with torch.cuda.graph(graph, stream=stream):
            yg = moe.forward(xd, ids, wts)
    torch.cuda.synchronize()
    u2 = 2 * ULP[dt]
    for r_ids, r_wts in routes[1:] + routes[:1]:
        ids.copy_(torch.from_numpy(r_ids))
        wts.copy_(torch.from_numpy(r_wts))
        graph.replay()
        torch.cuda.synchronize()
        got = host16(yg, dt)
        assert np.array_equal(got, host16(moe.forward(xd, ids, wts), dt))
        mm = G.round_dt(products(x, gu[2], r_ids, top_k), dt)
        act = G.silu_mul16(mm[:, :I], mm[:, I:], dt)
        down = r_wts.reshape(-1, 1) * products(act, dn[2], r_ids, 1)
        ref = G.round_dt(down, dt).astype(np.float64).reshape(T, top_k, H).sum(1)
        # act is within check_ulp(2.01, mag = up) of its reference (the SILU_MUL bound); that error goes through |down weights| times w_p;
        # each down row rounds once (1.01 ulp, the parity bound) and the f32 sum of top_k rows rounds once more
        act_tol = np.maximum(2.01 * u2 * np.maximum(np.abs(act), np.abs(mm[:, I:])), 1e-3 * np.abs(act).max() * ULP[dt] / ULP["bf16"])
        tol = np.abs(r_wts.reshape(-1, 1)) * products(act_tol, np.abs(dn[2]), r_ids, 1) + 1.01 * u2 * np.abs(down)
        tol = tol.reshape(T, top_k, H).sum(1) + 1.01 * u2 * np.abs(ref)
        assert np.isfinite(got).all() and (np.abs(got - ref) <= tol).all(), np.abs(got - ref).max()
