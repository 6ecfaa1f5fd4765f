"""The hand-counted `s_waitcnt vmcnt(N)` of the Q5_K arm of the LDS-fed prompt GEMM (csrc/qmm_prefill.inc: qpg_gemm_lds2_kernel<., false,
MI355_GGML_Q5_K>), checked against an in-order model of its instruction stream as tests/test_cpu_dma_plan.py does for the Q4_K arm.
Per wave and k-block the loop issues  I P1 P1 | I | I H Q S P0 P0 | I  behind the barriers of chunks 0..3 (I: image chunk, 3 ahead;
P1: plane 1 of THIS k-block; H, Q, S, P0: headers, fifth-bit words, sums and plane 0 of the NEXT one); prologue  I(0) | I(1) H Q S P0 P0 |
I(2).  Loads retire in order and `vmcnt(N)` retires all but the N issued last."""
import ctypes

import pytest

AFTER = {0: ["P1", "P1"], 1: [], 2: ["H", "Q", "S", "P0", "P0"], 3: []}      # weight DMAs behind the image DMA of chunk c


def _plan(lib):
    f = lib.mi355_internal_qpg_dma_plan
    f.restype, f.argtypes = ctypes.c_int32, [ctypes.c_int32, ctypes.c_void_p]
    out = (ctypes.c_int32 * 6)()
    assert f(5, ctypes.addressof(out)) == 0
    return list(out)


def _simulate(plan, nkb):
    lead, ring, xu, nw, ne, no = plan
    assert xu == 1 and nw == sum(len(v) for v in AFTER.values())
    issued, retired, slack = [], 0, []
    issued += [("I", 0), ("I", 1)] + [(k, 0) for k in AFTER[2]] + [("I", 2)]
    for kb in range(nkb):
        for c in range(4):
            kc, n = 4 * kb + c, (ne if c % 2 == 0 else no)
            retired = max(retired, len(issued) - n)                   # the counted wait in front of the chunk's barrier
            need = [("I", kc)] + ([("H", kb), ("Q", kb), ("S", kb), ("P0", kb)] if c == 0 else []) + ([("P1", kb)] if c == 2 else [])
            newest = max(i for i, op in enumerate(issued) if op in need)
            assert all(op in issued for op in need) and newest < retired, (nkb, kb, c)
            slack.append(len(issued) - 1 - newest - n)
            # behind the barrier: every wave has finished chunk kc - 1.  The image refill takes neither the slot being read nor an unconsumed one
            assert (kc + lead) % ring not in {(kc + d) % ring for d in range(lead)}
            issued.append(("I", kc + lead))                           # (past the end the kernel re-reads the last chunk into the same free slot)
            # single stages: plane 1 was last read in chunk 2 of kb - 1; plane 0, the headers and the fifth-bit words of kb went into
            # registers in chunk 0 of kb and are refilled in chunk 2; the sums (read in chunk 3 of kb) go to the other of their two stages
            issued += [(k, kb + (c == 2)) for k in AFTER[c]]
    return slack


def test_q5k_plan_is_exported_and_documented(lib):
    assert _plan(lib) == [3, 4, 1, 7, 1, 9]                           # ring of 4 chunks, 3 ahead, seven weight DMAs, vmcnt 1 (even) / 9 (odd)


@pytest.mark.parametrize("nkb", [1, 2, 3, 16, 56])
def test_q5k_counted_waits_are_safe_and_tight(lib, nkb):
    slack = _simulate(_plan(lib), nkb)
    assert min(slack) == 0, (nkb, slack[:12])                         # never negative, exact somewhere in every run
    if nkb == 16:
        assert set(slack[8:]) == {0}                                  # ... and everywhere in the steady state
