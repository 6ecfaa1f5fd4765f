"""`mi355_moe_gemm_fp8` (FusedMoeFp8, layers/moe.rs:1429-1481): what the host refuses before any device call, so it runs without a GPU.
REFUSALS is shared with tests/test_gpu_fp8_moe.py, which makes the same calls on real buffers and checks `out` afterwards."""
import ctypes

import pytest

INVALID, NOT_SUPPORTED = 1, 801                                # hipErrorInvalidValue, hipErrorNotSupported
BASE = dict(T=2, top_k=2, E=4, x_div=2, n=64, k=128, n_half=0, block_n=128, block_k=128, dtype=2, epi=0, wts=False, null=None)
REFUSALS = [("n % 16", dict(n=24)), ("k % 128", dict(k=192)), ("block_n 64", dict(block_n=64)), ("block_k 64", dict(block_k=64)),
            ("f32", dict(dtype=0)), ("4097 experts", dict(E=4097)), ("top_k 0", dict(top_k=0, x_div=0)), ("no expert", dict(E=0)),
            ("x_div 3", dict(x_div=3)), ("n_half 16", dict(n_half=16)), ("n_half % 16", dict(n=48, n_half=24)),
            ("silu_mul n % 32", dict(n=48, n_half=24, epi=2)), ("silu_mul with weights", dict(n_half=32, epi=2, wts=True)),
            ("silu_mul n_half 0", dict(epi=2)), ("resid epilogue", dict(epi=1)), ("null out", dict(null="out")),
            ("null x", dict(null="x")), ("null weights", dict(null="w")), ("null scales", dict(null="s")), ("null ids", dict(null="ids"))]
NAMES = ("out", "x", "w", "s", "ids", "wts")


def call(lib, ptr, **kw):
    """ptr: name -> address for out, x, w, s, ids, wts"""
    a = {**BASE, **kw}
    arg = {k: (None if a["null"] == k else v) for k, v in ptr.items()}
    return lib.mi355_moe_gemm_fp8(arg["out"], arg["x"], arg["w"], arg["s"], arg["ids"], arg["wts"] if a["wts"] else None, a["T"],
                                  a["top_k"], a["E"], a["x_div"], a["n"], a["k"], a["n_half"], a["block_n"], a["block_k"], a["dtype"],
                                  a["epi"], 0)


@pytest.mark.parametrize("what,kw", REFUSALS)
def test_moe_gemm_fp8_refuses_on_the_host(lib, what, kw):
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15                      # any aligned non-null pointer: the call must fail before using it
    assert call(lib, dict.fromkeys(NAMES, p), **kw) in (INVALID, NOT_SUPPORTED), what


def test_moe_gemm_fp8_without_tokens_is_a_no_op(lib):
    assert call(lib, dict.fromkeys(NAMES, None), T=0) == 0
    assert lib.mi355_moe_fp8_tile_repack(None, None, 0, 64, 128, 0) == INVALID
