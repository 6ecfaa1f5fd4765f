"""mi355_fp8_linear_tiled against mi355_linear_tiled (bf16) on the Llama-3-8B MLP shapes: gate|up (2 x 14336 x 4096, SILU_MUL) and down
(4096 x 14336, RESID) at 1, 32 and 2048 tokens.  Method of DESIGN.md section 5b: device events around back-to-back launches, the two
ops alternated in one process, three rounds, min - max per op; bytes = weight stream (+ scales), FLOP = 2 T N K.
    python tools/exp_fp8_linear.py [--out FILE] [--tokens 1,32,2048]
A build with another route (tools/build_variant_lib.sh with TU=fp8_linear and -DFP8_GEMM_MIN_T=n, loaded through MI355_LIB_PATH) runs
in a process of its own; its bf16 column is the yardstick that ties the two processes together."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import candle_vllm_amd.ops as cv                                                # noqa: E402


def timed(fn, iters):
    fn()                                                                        # warm-up: code object, lazily set attributes
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters                                    # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tokens", default="1,32,2048")
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for name, N, K, epi in (("gate_up", 2 * 14336, 4096, cv.EPI_SILU_MUL), ("down", 4096, 14336, cv.EPI_RESID)):
        w16 = (torch.randn((N, K), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
        w8 = torch.randint(0, 0x7F, (N, K), generator=g, device="cuda", dtype=torch.uint8)       # finite positive codes
        sc = torch.rand((N // 128, K // 128), generator=g, device="cuda") * 2.0 ** -9 + 2.0 ** -10
        dense, fp8 = cv.Linear(w16, tiled=True), cv.Fp8Linear(w8, sc)
        del w16, w8
        for T in [int(t) for t in args.tokens.split(",")]:
            x = torch.randn((T, K), generator=g, device="cuda").to(torch.bfloat16)
            n_out = N // 2 if epi == cv.EPI_SILU_MUL else N
            res = torch.zeros((T, n_out), dtype=torch.bfloat16, device="cuda") if epi == cv.EPI_RESID else None
            out = torch.empty((T, n_out), dtype=torch.bfloat16, device="cuda")
            iters = 200 if T <= 32 else 30
            t = {"bf16": [], "fp8": []}
            for _ in range(3):                                                  # alternated: both ops see the same neighbours on the machine
                t["bf16"].append(timed(lambda: dense.forward(x, epilogue=epi, residual=res, out=out), iters))
                t["fp8"].append(timed(lambda: fp8.forward(x, epilogue=epi, residual=res, out=out), iters))
            row = {"proj": name, "T": T, "N": N, "K": K}
            for k, bpw in (("bf16", 2.0), ("fp8", 1.0)):
                lo, hi = min(t[k]), max(t[k])
                row[k + "_us"] = [round(lo, 2), round(hi, 2)]
                row[k + "_weight_TBps"] = round(N * K * bpw / lo * 1e-6, 3)
                row[k + "_TFLOPs"] = round(2.0 * T * N * K / lo * 1e-6, 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
