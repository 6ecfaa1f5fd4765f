"""mi355_moe_gemm_fp8 against what the library offered before it: the routing copied to the host, sorted there, and one
mi355_fp8_linear_tiled per expert with its gather and scatter in torch.  Qwen3-30B-A3B's experts (E = 128, top_k = 8, hidden 2048,
intermediate 768): gate|up (1536 x 2048, SILU_MUL, one x row per token) and down (2048 x 768, weighted, one x row per pair).  Method of
DESIGN.md 5b / 5d: device events around back-to-back calls, the candidates alternated in one process, three rounds, min - max.
    python tools/exp_fp8_moe.py [--out FILE] [--tokens 1,32,2048] [--dtypes bf16,f16] [--no-loop]
A build with another route edge (TU=fp8_moe bash tools/build_variant_lib.sh name -DFP8MOE_GEMM_MIN_AVG=n, loaded through
MI355_LIB_PATH) runs in a process of its own with --no-loop."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import candle_vllm_amd.ops as cv                                                # noqa: E402

E, TOP_K, H, I = 128, 8, 2048, 768


def timed(fn, iters):
    fn()                                                                        # warm-up: code object, scratch growth
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters                                    # us per call


def loop(lins, x, ids, wts, x_div, epi, out):
    """the host-sorted per-expert loop: one device -> host copy of the routing, then gather, linear, (weight,) scatter per expert"""
    flat = ids.reshape(-1).cpu()
    order = torch.argsort(flat, stable=True)
    counts = torch.bincount(flat, minlength=len(lins)).tolist()
    order, at = order.cuda(), 0
    for e, c in enumerate(counts):
        if c:
            rows = order[at:at + c]
            y = lins[e].forward(x.index_select(0, rows // x_div), epilogue=epi)
            out[rows] = y if wts is None else (y.float() * wts.reshape(-1, 1)[rows]).to(y.dtype)
            at += c
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tokens", default="1,32,2048")
    ap.add_argument("--dtypes", default="bf16,f16")
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8, device="cuda")     # the finite e4m3fn codes
    weight, scale = {}, {}
    for which, n, k in (("gate_up", 2 * I, H), ("down", H, I)):                 # (I = 768 = 6 x 128: cat(gate, up) scale rows == the plain rows)
        weight[which] = codes[torch.randint(0, len(codes), (E, n, k), generator=g, device="cuda")]
        scale[which] = (0.5 + torch.rand((E, n // 128, k // 128), generator=g, device="cuda")) * 2.0 ** -9
    moe = cv.Fp8MoE(weight["gate_up"], scale["gate_up"], weight["down"], scale["down"])
    lins = {w: [cv.Fp8Linear(weight[w][e], scale[w][e]) for e in range(E)] for w in weight} if not args.no_loop else None
    rows = []
    for dt in [{"bf16": torch.bfloat16, "f16": torch.float16}[d] for d in args.dtypes.split(",")]:
        for T in [int(t) for t in args.tokens.split(",")]:
            ids = torch.rand((T, E), generator=g, device="cuda").topk(TOP_K, dim=1).indices.to(torch.int32)
            wts = torch.rand((T, TOP_K), generator=g, device="cuda")
            for which, n, k, x_rows, epi, w in (("gate_up", 2 * I, H, T, cv.EPI_SILU_MUL, None), ("down", H, I, T * TOP_K, cv.EPI_STORE, wts)):
                x = (torch.randn((x_rows, k), generator=g, device="cuda") * 0.1).to(dt)
                n_out = n // 2 if epi == cv.EPI_SILU_MUL else n
                out = torch.empty((T * TOP_K, n_out), dtype=dt, device="cuda")
                ops = {"fused": lambda: moe.gemm(x, ids, which=which, topk_weights=w, epilogue=epi, out=out)}
                if lins:
                    ref = torch.empty_like(out)
                    ops["loop"] = lambda: loop(lins[which], x, ids, w, TOP_K if which == "gate_up" else 1, epi, ref)
                iters = {"fused": 200 if T <= 32 else 30, "loop": 20 if T <= 32 else 5}
                t = {k_: [] for k_ in ops}
                for _ in range(3):                                              # alternated: the candidates see the same neighbours
                    for k_, fn in ops.items():
                        t[k_].append(timed(fn, iters[k_]))
                row = {"proj": which, "dtype": str(dt).split(".")[-1], "T": T, "pairs_per_expert": T * TOP_K / E}
                for k_ in ops:
                    row[k_ + "_us"] = [round(min(t[k_]), 2), round(max(t[k_]), 2)]
                # bytes the call must read (the weights of the experts hit, once) and its FLOP, from the shapes
                hit = int(torch.unique(ids).numel())
                row["weight_GB_per_s"] = round(hit * n * k / min(t["fused"]) * 1e-3, 1)
                row["TFLOP_per_s"] = round(2.0 * T * TOP_K * n * k / min(t["fused"]) * 1e-6, 2)
                if lins:                                                        # gate|up: the same roundings; down: the loop rounds before w_p
                    row["max_abs_diff"] = float((out.float() - ref.float()).abs().max())
                    row["differing"] = int((out != ref).sum())
                    row["out_abs_max"] = float(ref.float().abs().max())
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
