"""`mi355_moe_gemm_mxfp4` (FusedMoeMxfp4, layers/moe.rs:1782-1835): what the host refuses before any device call, so it runs without a
GPU.  REFUSALS is shared with tests/test_gpu_mxfp4_moe.py, which makes the same calls on real buffers and checks `out` afterwards."""
import ctypes

import pytest

INVALID, NOT_SUPPORTED = 1, 801                                # hipErrorInvalidValue, hipErrorNotSupported
BASE = dict(T=2, top_k=2, E=4, x_div=2, n=64, k=128, group=32, dtype=2, epi=0, wts=False, null=None)
REFUSALS = [("n % 16", dict(n=24)), ("k % 128", dict(k=192)), ("group 16", dict(group=16)), ("f32", dict(dtype=0)),
            ("top_k 0", dict(top_k=0, x_div=0)), ("no expert", dict(E=0)), ("x_div 3", dict(x_div=3)),
            ("silu_mul n % 32", dict(n=48, epi=2)), ("silu_mul with weights", dict(epi=2, wts=True)), ("resid epilogue", dict(epi=1)),
            ("null out", dict(null="out")), ("null x", dict(null="x")), ("null blocks", dict(null="w")), ("null scales", dict(null="s")),
            ("null ids", dict(null="ids"))]


def call(lib, ptr, **kw):
    """ptr: name -> address for out, x, w, s, ids, wts"""
    a = {**BASE, **kw}
    arg = {k: (None if a["null"] == k else v) for k, v in ptr.items()}
    return lib.mi355_moe_gemm_mxfp4(arg["out"], arg["x"], arg["w"], arg["s"], arg["ids"], arg["wts"] if a["wts"] else None, a["T"],
                                    a["top_k"], a["E"], a["x_div"], a["n"], a["k"], a["group"], a["dtype"], a["epi"], 0)


@pytest.mark.parametrize("what,kw", REFUSALS)
def test_moe_gemm_mxfp4_refuses_on_the_host(lib, what, kw):
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15                      # any aligned non-null pointer: the call must fail before using it
    assert call(lib, dict.fromkeys(("out", "x", "w", "s", "ids", "wts"), p), **kw) in (INVALID, NOT_SUPPORTED), what


def test_moe_gemm_mxfp4_without_tokens_is_a_no_op(lib):
    assert call(lib, dict.fromkeys(("out", "x", "w", "s", "ids", "wts"), None), T=0) == 0
    assert lib.mi355_moe_mxfp4_tile_repack(None, None, None, None, 0, 64, 128, 0) == INVALID
