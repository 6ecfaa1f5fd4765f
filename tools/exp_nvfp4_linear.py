"""mi355_nvfp4_linear_tiled against mi355_mxfp4_linear_tiled, mi355_fp8_linear_tiled and mi355_linear_tiled (16-bit) on the Llama-3-8B
MLP shapes: gate|up (2 x 14336 x 4096, SILU_MUL) and down (4096 x 14336, RESID) at 1, 17, 32, 33, 64, 96, 128 and 2048 tokens, bf16 and
f16.  Method of DESIGN.md section 5b - 5d: device events around back-to-back launches, the four ops alternated in one process, three rounds,
min - max per op; bytes = weight stream (+ scales), FLOP = 2 T N K.  Back-to-back launches re-read the same weights and these matrices
fit the last-level cache: the TB/s are rates of this harness, not of HBM.
    python tools/exp_nvfp4_linear.py [--out FILE] [--tokens 1,32,2048] [--dtypes bf16,f16] [--cvt-probe]
A build with another route (TU=nvfp4_linear bash tools/build_variant_lib.sh name -DNVFP4_GEMM_MIN_T=n or -DNVFP4_GEMM_MIN_WGS=n, loaded
through MI355_LIB_PATH) runs in a process of its own; its 16-bit, fp8 and mxfp4 columns are the yardsticks that tie the processes together.
--cvt-probe first runs tools/probe_fp4_cvt_scale.hip (built into build_variant/ when it is not there yet): the bit-level answer to whether
the fp4 convert instructions honour the mantissa of their scale operand."""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import candle_vllm_amd.ops as cv                                                # noqa: E402


def cvt_probe():
    exe = os.path.join(ROOT, "build_variant", "probe_fp4_cvt_scale")
    if not os.path.exists(exe):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O2",
                        os.path.join(ROOT, "tools", "probe_fp4_cvt_scale.hip"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True, timeout=120, check=True)   # a fresh process: this one holds the GPU
    print(r.stdout.strip(), flush=True)
    return json.loads(r.stdout)


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
    ap.add_argument("--tokens", default="1,17,32,33,64,96,128,2048")
    ap.add_argument("--dtypes", default="bf16,f16")
    ap.add_argument("--cvt-probe", action="store_true")
    args = ap.parse_args()
    rows = [cvt_probe()] if args.cvt_probe else []
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, N, K, epi in (("gate_up", 2 * 14336, 4096, cv.EPI_SILU_MUL), ("down", 4096, 14336, cv.EPI_RESID)):
        w8 = torch.randint(0, 0x7F, (N, K), generator=g, device="cuda", dtype=torch.uint8)       # finite positive e4m3 codes
        sc = torch.rand((N // 128, K // 128), generator=g, device="cuda") * 2.0 ** -9 + 2.0 ** -10
        fp8 = cv.Fp8Linear(w8, sc)
        w4 = torch.randint(0, 256, (N, K // 2), generator=g, device="cuda", dtype=torch.uint8)   # all 16 codes
        mx4 = cv.Mxfp4Linear(w4, torch.randint(112, 122, (N, K // 32), generator=g, device="cuda", dtype=torch.uint8))
        # e4m3 codes 0x08 .. 0x47 (2^-6 .. 1.875): with the 2^-3 global scales the weights are of the size of the other columns'
        nv4 = cv.Nvfp4Linear(w4, torch.randint(0x08, 0x48, (N, K // 16), generator=g, device="cuda", dtype=torch.uint8), 0.125,
                             global_scale_up=0.11)
        del w8, w4
        for dt in [{"bf16": torch.bfloat16, "f16": torch.float16}[d] for d in args.dtypes.split(",")]:
            dense = cv.Linear((torch.randn((N, K), generator=g, device="cuda") * 0.02).to(dt), tiled=True)
            for T in [int(t) for t in args.tokens.split(",")]:
                x = torch.randn((T, K), generator=g, device="cuda").to(dt)
                n_out = N // 2 if epi == cv.EPI_SILU_MUL else N
                res = torch.zeros((T, n_out), dtype=dt, device="cuda") if epi == cv.EPI_RESID else None
                out = torch.empty((T, n_out), dtype=dt, device="cuda")
                iters = 200 if T <= 32 else 30
                ops = {"dense": (dense, 2.0), "fp8": (fp8, 1.0 + 4.0 / 16384), "mxfp4": (mx4, 0.5 + 1.0 / 32), "nvfp4": (nv4, 0.5 + 1.0 / 16)}
                t = {k: [] for k in ops}
                for _ in range(3):                                              # alternated: the ops see the same neighbours on the machine
                    for k, (op, _) in ops.items():
                        t[k].append(timed(lambda: op.forward(x, epilogue=epi, residual=res, out=out), iters))
                row = {"proj": name, "dtype": str(dt).split(".")[-1], "T": T, "N": N, "K": K}
                for k, (_, bpw) in ops.items():
                    lo, hi = min(t[k]), max(t[k])
                    row[k + "_us"] = [round(lo, 2), round(hi, 2)]
                    row[k + "_weight_TBps"] = round(N * K * bpw / lo * 1e-6, 3)
                    row[k + "_TFLOPs"] = round(2.0 * T * N * K / lo * 1e-6, 1)
                rows.append(row)
                print(json.dumps(row), flush=True)
            del dense
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
