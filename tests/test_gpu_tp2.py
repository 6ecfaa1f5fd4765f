"""Two tensor-parallel RANKS on ONE GPU: two processes, each with its shard of the model in the library's C++ host
layer, collectives supplied by the host (`mi355_comm_create_external`) over a gloo process group that stages the
payload through host memory.  This runs the real multi-rank host logic -- shard shapes, residual placement around the
all-reduce, vocab-parallel gather + transpose, greedy sampling over the gathered vocabulary -- on a single-GPU box;
the RCCL transport itself is covered by the 1-rank communicator tests."""
import os
import socket

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.multiprocessing as mp                      # noqa: E402

from oracle import llama                                # noqa: E402
from oracle import dense_llama as DL                    # noqa: E402
from oracle import ops as O                             # noqa: E402

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gguf_case(moe=False, vocab=512):
    cfg = llama.LlamaConfig.tiny(hidden=512, n_heads=4, n_kv_heads=2, head_dim=128, intermediate=1024, vocab=vocab)
    if moe:                                              # Mixtral shape: experts replicated, attention sharded
        cfg.n_expert, cfg.n_expert_used = 4, 2
        W = llama.make_moe_weights(cfg, 4, seed=99)
    else:
        W = llama.make_weights(cfg, seed=99)
    rng = np.random.default_rng(5)
    seqs = [{"tokens": [int(t) for t in rng.integers(0, cfg.vocab, 21)], "block_table": [2, 5]},
            {"tokens": [int(t) for t in rng.integers(0, cfg.vocab, 9)], "block_table": [1]}]
    return cfg, W, seqs


def _gguf_worker(rank, world, port, q, moe=False, p2p=False, wire=0, vocab=512):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from candle_vllm_amd import model as M, tp
    cfg, W, seqs = _gguf_case(moe, vocab)
    comm = tp.TorchDistComm()
    if p2p:
        comm.attach_p2p()                                # decode-sized all-reduces: the one-shot peer kernel (IPC regions)
    comm.set_options(1, wire)
    gm = M.GGUFLLaMa(cfg, max_batch=2, kv_layout=M.KV_PAGED, tp_rank=rank, tp_world=world)
    gm.load_oracle_weights(tp.shard_weights(W, cfg, rank, world))
    gm.alloc_kv_cache(8)
    gm.set_comm(comm.handle)
    pre = gm.forward_prefill(O.prepare_prompt(seqs, cfg.block_size)).cpu().numpy()
    for s, row in zip(seqs, pre):
        s["tokens"].append(int(row.argmax()))
    dec = gm.forward_decode(O.prepare_decode(seqs, cfg.block_size)).cpu().numpy()
    # the C++ greedy loop (argmax over the GATHERED vocabulary, device-side input advance), 3 steps, eager under TP
    for s, extra in zip(seqs, (3, 4)):
        s["block_table"] = s["block_table"] + [extra]
    bt = np.zeros((2, 3), np.uint32)
    for i, s in enumerate(seqs):
        bt[i, :len(s["block_table"])] = s["block_table"]
    stream = torch.cuda.Stream()
    gm.decode_begin([s["tokens"][-1] for s in seqs], [len(s["tokens"]) for s in seqs], bt,
                    ctx_cap=max(len(s["tokens"]) for s in seqs) + 4, stream=stream.cuda_stream)
    toks = []
    for _ in range(3):
        gm.decode_step(stream.cuda_stream)
        toks.append([int(t) for t in gm.read_tokens(stream.cuda_stream)])
    q.put((rank, pre, dec, toks, M.lib.mi355_comm_p2p_error(comm.handle)))
    dist.barrier()
    comm.close()
    dist.destroy_process_group()


class _LockstepComm:
    """two oracle ranks in two threads of this process: all_reduce / all_gather meet at a barrier.  wire = 1: the
    reference's all-reduce dtype -- every partial rounded to bf16, bf16 sum (attention.rs:1003-1008)"""

    def __init__(self, world, wire):
        import threading
        self.world, self.wire = world, wire
        self.slots = [None] * world
        self.bar = threading.Barrier(world)

    def view(self, rank):
        outer = self

        class _V:
            def all_reduce(self, x):
                outer.slots[rank] = np.asarray(x, np.float32)
                outer.bar.wait()
                parts = [O.round_bf16(p) if outer.wire else p for p in outer.slots]
                tot = parts[0].copy()
                for p in parts[1:]:
                    tot = tot + p
                if outer.wire:
                    tot = O.round_bf16(tot)
                outer.bar.wait()
                return tot

            def all_gather(self, x):
                outer.slots[rank] = np.asarray(x)
                outer.bar.wait()
                out = [p.copy() for p in outer.slots]
                outer.bar.wait()
                return out
        return _V()


def _oracle_two_ranks(cfg, W, seqs, wire):
    """the 2-rank ORACLE (shards of candle_vllm_amd/tp.py, collectives in the requested wire dtype): prompt step + one
    decode step, as rank 0 sees them"""
    import threading
    from candle_vllm_amd import tp
    lc = _LockstepComm(2, wire)
    out = [None, None]

    def run(rank):
        orc = llama.OracleLlama(tp.shard_config(cfg, rank, 2), tp.shard_weights(W, cfg, rank, 2), flash_layout=False, comm=lc.view(rank))
        cache = orc.new_cache(8)
        sq = [{"tokens": list(s["tokens"]), "block_table": list(s["block_table"])} for s in seqs]
        pre = orc.forward(O.prepare_prompt(sq, cfg.block_size), cache, is_prefill=True)
        for s, row in zip(sq, pre):
            s["tokens"].append(int(row.argmax()))
        dec = orc.forward(O.prepare_decode(sq, cfg.block_size), cache)
        out[rank] = (pre, dec)
    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return out[0]


@pytest.mark.parametrize("moe,p2p,wire,vocab", [(False, False, 0, 512), (True, False, 0, 512), (False, True, 0, 512), (False, True, 1, 512),
                                                 (False, False, 1, 512), (False, False, 0, 500), (False, True, 0, 785)])
def test_gguf_tp2_two_ranks_on_one_gpu_equal_the_unsharded_model(lib, moe, p2p, wire, vocab):
    """p2p: the all-reduces of the step go through the one-shot peer kernel (two processes, one GPU, IPC-opened regions);
    wire = 1: the reference's bf16 wire numerics (attention.rs:1003-1008) -- both against the UNSHARDED oracle (the bf16
    wire rounds each partial once more: same 3e-3 band).  vocab = 500 / 785: vocabularies `pad_vocab_size` pads (a GPT-2-style
    50257 in small: odd, -> 512 / 832): the lm_head shards carry zero rows, the gathered logits are narrowed back and the greedy
    loop samples over the real vocabulary only (VocabParallelLinear, distributed.rs:1448-1454,1596-1616,1657-1660)"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    cfg, W, seqs = _gguf_case(moe, vocab)
    wire_ref = _oracle_two_ranks(cfg, W, seqs, 1) if wire else None    # the reference's numerics, restated on two oracle ranks
    orc = llama.OracleLlama(cfg, W, flash_layout=False)
    cache = orc.new_cache(8)
    pre = orc.forward(O.prepare_prompt(seqs, cfg.block_size), cache, is_prefill=True)
    for s, row in zip(seqs, pre):
        s["tokens"].append(int(row.argmax()))
    dec = orc.forward(O.prepare_decode(seqs, cfg.block_size), cache)
    want = []
    for s, extra in zip(seqs, (3, 4)):
        s["block_table"] = s["block_table"] + [extra]
    o_seqs = [{"tokens": list(s["tokens"]), "block_table": list(s["block_table"])} for s in seqs]
    # the device loop's first step recomputes the decode step above (same cache slot), then advances
    for _ in range(3):
        lg = orc.forward(O.prepare_decode(o_seqs, cfg.block_size), cache)
        nxt = [int(r.argmax()) for r in lg]
        want.append(nxt)
        for s, t in zip(o_seqs, nxt):
            s["tokens"].append(t)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gguf_worker, args=(r, 2, port, q, moe, p2p, wire, vocab)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(2):
        r = q.get(timeout=300)
        res[r[0]] = r[1:]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank in (0, 1):                                   # every rank ends up with the full logits
        got_pre, got_dec, toks, p2p_err = res[rank]
        assert p2p_err == 0                               # no peer wait ran into its spin bound
        assert got_pre.shape == pre.shape and got_dec.shape == dec.shape and pre.shape[-1] == vocab
        if wire:
            # The bf16 wire moves the logits ~3e-3 of their scale away from the unsharded f32 model (the 2-rank ORACLE with
            # the same wire: 2.97e-3), and which partials round up or down flips on 1e-6 differences between two correct
            # implementations -- so the GPU sits about as far from the wire oracle as from the unsharded one (measured
            # 4.1e-3 / 3.5e-3).  The wire arithmetic itself is pinned bit for bit at the op level
            # (test_one_shot_peer_all_reduce_two_processes_one_gpu); here: the band, on both references.
            rp, rd = wire_ref
            assert np.abs(got_pre - rp).max() < 8e-3 * np.abs(rp).max()
            assert np.abs(got_dec - rd).max() < 8e-3 * np.abs(rd).max()
            assert np.abs(got_pre - pre).max() < 8e-3 * np.abs(pre).max()
            continue
        assert np.abs(got_pre - pre).max() < 3e-3 * np.abs(pre).max()
        assert np.abs(got_dec - dec).max() < 3e-3 * np.abs(dec).max()
        assert toks == want, (rank, toks, want)
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def _dense_case(gptq, vocab=512):
    cfg = DL.DenseConfig(hidden=512, n_layers=2, n_heads=8, n_kv_heads=2, head_dim=64, intermediate=1024, vocab=vocab,
                         rope_theta=10000.0, max_seq=256, block_size=16, qkv_bias=True)
    W = DL.make_weights(cfg, seed=31)
    if gptq:
        W = DL.quantize_gptq(W, group=128)
    rng = np.random.default_rng(8)
    seqs = [{"tokens": [int(t) for t in rng.integers(0, cfg.vocab, 19)], "block_table": [3, 1]},
            {"tokens": [int(t) for t in rng.integers(0, cfg.vocab, 7)], "block_table": [2]}]
    return cfg, W, seqs


def _dense_worker(rank, world, port, q, gptq, vocab=512):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from candle_vllm_amd import dense_model as M, tp
    cfg, W, seqs = _dense_case(gptq, vocab)
    comm = tp.TorchDistComm()
    gm = M.DenseLlama(tp.shard_dense_config(cfg, rank, world), max_batch=4, kv_layout=M.KV_PAGED, tp_rank=rank, tp_world=world)
    gm.load_oracle_weights(tp.shard_dense_weights(W, cfg, rank, world))
    gm.alloc_kv_cache(8)
    gm.set_comm(comm.handle)
    pre = gm.forward(O.prepare_prompt(seqs, cfg.block_size), is_prefill=True).cpu().numpy()
    for s, row in zip(seqs, pre):
        s["tokens"].append(int(row.argmax()))
    dec = gm.forward(O.prepare_decode(seqs, cfg.block_size)).cpu().numpy()
    # the C++ greedy loop (argmax over the gathered row NARROWED to the real vocabulary), 2 steps, eager under host collectives
    for s, row in zip(seqs, dec):
        s["tokens"].append(int(row.argmax()))
    maxb = max(len(s["block_table"]) for s in seqs)
    bt = np.zeros((len(seqs), maxb), np.uint32)
    for i, s in enumerate(seqs):
        bt[i, :len(s["block_table"])] = s["block_table"]
    gm.decode_begin([s["tokens"][-1] for s in seqs], [len(s["tokens"]) for s in seqs], bt, ctx_cap=max(len(s["tokens"]) for s in seqs) + 3)
    toks = []
    for _ in range(2):
        gm.decode_step(0)
        toks.append(gm.read_tokens(0).tolist())
    q.put((rank, pre, dec, toks, gm.loop_logits().cpu().numpy()))
    dist.barrier()
    comm.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("gptq,vocab", [(False, 512), (True, 512), (False, 500)])
def test_dense_tp2_two_ranks_on_one_gpu(lib, gptq, vocab):
    """16-bit / GPTQ host path (BASELINE config 4 is Qwen2 GPTQ at TP=2): the 2-rank device run must agree with the
    unsharded oracle to 16-bit accumulation noise and pick the same tokens (the row-parallel partial products are rounded
    per rank before the sum, so TP=2 is not bit-identical to TP=1 -- tests/test_cpu_tp.py shows the same for the oracle).
    vocab = 500: a vocabulary `pad_vocab_size` pads to 512 -- rank 1's lm_head shard ends in 12 zero rows, logits rows and the greedy loop's
    argmax are narrowed to 500 columns (mi355_dense_config.vocab_total; VocabParallelLinear, distributed.rs:1657-1663)."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    cfg, W, seqs = _dense_case(gptq, vocab)
    orc = DL.OracleDenseLlama(cfg, W, flash_layout=False)
    cache = orc.new_cache(8)
    pre = orc.forward(O.prepare_prompt(seqs, cfg.block_size), cache, is_prefill=True)
    for s, row in zip(seqs, pre):
        s["tokens"].append(int(row.argmax()))
    dec = orc.forward(O.prepare_decode(seqs, cfg.block_size), cache)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dense_worker, args=(r, 2, port, q, gptq, vocab)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(2):
        r = q.get(timeout=300)
        res[r[0]] = r[1:]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank in (0, 1):
        got_pre, got_dec, toks, loop_lg = res[rank]
        assert got_pre.shape == pre.shape and got_dec.shape == dec.shape and pre.shape[-1] == vocab
        assert np.abs(got_pre - pre).max() < 3e-2 * np.abs(pre).max()
        assert np.abs(got_dec - dec).max() < 3e-2 * np.abs(dec).max()
        assert (got_pre.argmax(-1) == pre.argmax(-1)).all()
        assert loop_lg.shape[-1] * 0 == 0 and loop_lg.size == len(seqs) * vocab
        assert all(0 <= t < vocab for step in toks for t in step), toks
        # the loop's last logits row is the device's own argmax input: its token is the row's first maximum over the REAL vocabulary
        assert toks[-1] == [int(r.argmax()) for r in loop_lg.reshape(len(seqs), vocab)]
    assert np.array_equal(res[0][0], res[1][0]) and res[0][2] == res[1][2]


def _unaligned_case():
    """H = 6 heads over 2 ranks -> 3 local heads: o_proj shard = 384 columns, down_proj shard = 384 columns: both cut a 256-wide
    k-quant block -> the reference's Q8_0 re-quantising fallback (quantized_var_builder.rs:234-269)"""
    cfg = llama.LlamaConfig.tiny(hidden=512, n_heads=6, n_kv_heads=2, head_dim=128, intermediate=768, vocab=512)
    W = llama.make_weights(cfg, seed=77)
    rng = np.random.default_rng(6)
    seqs = [{"tokens": [int(t) for t in rng.integers(0, cfg.vocab, 21)], "block_table": [2, 5]},
            {"tokens": [int(t) for t in rng.integers(0, cfg.vocab, 9)], "block_table": [1]}]
    return cfg, W, seqs


def _gguf_file_worker(rank, world, port, q, path, unaligned=False, vocab=512):
    try:
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.cuda.set_device(0)
        from candle_vllm_amd import model as M, tp
        from oracle import kquants as kq
        cfg, W, seqs = _unaligned_case() if unaligned else _gguf_case(False, vocab)
        W = dict(W)
        W["tok_embd"] = kq.dequantize_q6_k(kq.quantize(W["tok_embd"], kq.GGML_Q6_K)).reshape(cfg.vocab, cfg.hidden).astype(np.float32)
        # both models are built before the first collective, so a loader error cannot leave the peer waiting
        a = M.GGUFLLaMa.from_gguf(path, max_batch=2, max_blocks_per_seq=16, block_size=cfg.block_size,
                                  kv_layout=M.KV_PAGED, tp_rank=rank, tp_world=world)
        b = M.GGUFLLaMa(cfg, max_batch=2, max_blocks_per_seq=16, kv_layout=M.KV_PAGED, tp_rank=rank, tp_world=world)
        b.load_oracle_weights(tp.shard_weights(W, cfg, rank, world, kq.requantize_shard_q8_0))
        dims = (a.c.hidden, a.c.n_heads, a.c.n_kv_heads, a.c.intermediate, a.c.vocab, a.c.tp_rank, a.c.tp_world)
        comm = tp.TorchDistComm()
        meta = O.prepare_prompt(seqs, cfg.block_size)
        outs = []
        for m in (a, b):
            m.alloc_kv_cache(8)
            m.set_comm(comm.handle)
            outs.append(m.forward_prefill(meta).cpu().numpy())
        q.put((rank, "ok", dims, outs[0], outs[1]))
        dist.barrier()
        comm.close()
        dist.destroy_process_group()
    except Exception as e:                                 # reported to the parent, which stops both ranks
        q.put((rank, "error", repr(e)))
        raise


@pytest.mark.parametrize("vocab", [512, 500])
def test_gguf_file_loader_tp2_equals_setter_shards(lib, tmp_path, vocab):
    """f3 'TP re-sharding': every rank opens the same GGUF file through `mi355_llama_load_gguf_tp` and keeps its raw
    byte-range shard (get_sharded_no_shape, quantized_var_builder.rs:222-233); the prompt-step logits must be
    bit-identical to the model whose shards were cut by candle_vllm_amd/tp.py and handed over through the setters, and
    agree with the unsharded oracle.  vocab = 500: the loader pads the lm_head shards with zero rows (-> 512)."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from oracle import gguf_writer as GW
    from oracle import kquants as kq
    cfg, W, seqs = _gguf_case(False, vocab)
    W = dict(W)
    W["tok_embd"] = kq.dequantize_q6_k(kq.quantize(W["tok_embd"], kq.GGML_Q6_K)).reshape(cfg.vocab, cfg.hidden).astype(np.float32)
    path = os.path.join(tmp_path, "tp2.gguf")
    GW.llama_to_gguf(path, cfg, W)
    orc = llama.OracleLlama(cfg, W, flash_layout=False)
    ref = orc.forward(O.prepare_prompt(seqs, cfg.block_size), orc.new_cache(8), is_prefill=True)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gguf_file_worker, args=(r, 2, port, q, path, False, vocab)) for r in range(2)]
    for p in procs:
        p.start()
    res, err = {}, None
    try:
        for _ in range(2):
            r = q.get(timeout=300)
            if r[1] == "error":
                err = r
                break
            res[r[0]] = r[2:]
    finally:
        for p in procs:
            p.join(timeout=5 if err else 120)
            if p.is_alive():
                p.terminate()                              # this test's own children only
    assert err is None, err
    for rank in (0, 1):
        dims, from_file, from_setters = res[rank]
        assert dims == (cfg.hidden, cfg.n_heads, cfg.n_kv_heads, cfg.intermediate, cfg.vocab, rank, 2)   # GLOBAL dims
        assert np.array_equal(from_file, from_setters)
        assert np.abs(from_file - ref).max() < 3e-3 * np.abs(ref).max()


def test_gguf_file_loader_tp2_requantises_unaligned_shards_to_q8_0(lib, tmp_path):
    """`get_sharded_no_shape`'s fallback (quantized_var_builder.rs:234-269) on the device: o_proj / down_proj shards of 384
    columns are dequantised, narrowed and re-quantised to Q8_0 by the loader and multiplied by the Q8_0 arm.  The loaded
    model is bit-identical to the one whose shards the test cut itself (same bytes, checked on the CPU in
    test_cpu_gguf.py) and agrees with the 2-rank ORACLE over the same re-quantised shards."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import threading
    from candle_vllm_amd import tp
    from oracle import gguf_writer as GW
    from oracle import kquants as kq
    cfg, W, seqs = _unaligned_case()
    W = dict(W)
    W["tok_embd"] = kq.dequantize_q6_k(kq.quantize(W["tok_embd"], kq.GGML_Q6_K)).reshape(cfg.vocab, cfg.hidden).astype(np.float32)
    path = os.path.join(tmp_path, "q8.gguf")
    GW.llama_to_gguf(path, cfg, W)
    lc = _LockstepComm(2, 0)
    refs = [None, None]

    def run(rank):
        orc = llama.OracleLlama(tp.shard_config(cfg, rank, 2), tp.shard_weights(W, cfg, rank, 2, kq.requantize_shard_q8_0),
                                flash_layout=False, comm=lc.view(rank))
        refs[rank] = orc.forward(O.prepare_prompt(seqs, cfg.block_size), orc.new_cache(8), is_prefill=True)
    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gguf_file_worker, args=(r, 2, port, q, path, True)) for r in range(2)]
    for p in procs:
        p.start()
    res, err = {}, None
    try:
        for _ in range(2):
            r = q.get(timeout=300)
            if r[1] == "error":
                err = r
                break
            res[r[0]] = r[2:]
    finally:
        for p in procs:
            p.join(timeout=5 if err else 120)
            if p.is_alive():
                p.terminate()                              # this test's own children only
    assert err is None, err
    for rank in (0, 1):
        dims, from_file, from_setters = res[rank]
        assert dims == (cfg.hidden, cfg.n_heads, cfg.n_kv_heads, cfg.intermediate, cfg.vocab, rank, 2)
        assert np.array_equal(from_file, from_setters)
        assert np.abs(from_file - refs[0]).max() < 3e-3 * np.abs(refs[0]).max()


# ------------------------------------------------------------------------------------------------ one-shot peer all-reduce
def _p2p_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from candle_vllm_amd import tp
    from candle_vllm_amd._lib import lib
    comm = tp.TorchDistComm()
    comm.attach_p2p()
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    out = {}
    with torch.cuda.stream(stream):
        # (a) plain in-place f32 sums of several sizes, several calls each (sequence numbers / both parities)
        for n in (100, 4096, 5000, 16384, 65536):
            for it in range(4):
                x = torch.from_numpy(np.random.default_rng(1000 * n + 10 * it + rank).standard_normal(n).astype(np.float32)).cuda()
                assert lib.mi355_comm_all_reduce(comm.handle, x.data_ptr(), n, 0, st) == 0
                torch.cuda.synchronize()
                out[("sum", n, it)] = x.cpu().numpy()
        # (b) the same kernel replayed from a hipGraph (sequence numbers live on the device)
        n = 4096
        buf = torch.zeros(n, dtype=torch.float32, device="cuda")
        src = [torch.from_numpy(np.random.default_rng(77 + 10 * it + rank).standard_normal(n).astype(np.float32)).cuda() for it in range(3)]
        buf.copy_(src[0])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            assert lib.mi355_comm_all_reduce(comm.handle, buf.data_ptr(), n, 0, torch.cuda.current_stream().cuda_stream) == 0
        for it in range(3):
            buf.copy_(src[it])
            torch.cuda.synchronize()
            dist.barrier()
            g.replay()
            torch.cuda.synchronize()
            out[("graph", it)] = buf.cpu().numpy()
        # (c) the reference's wire numerics: resid += bf16(sum_r bf16(y_r))
        comm.set_options(1, 1)
        n = 8192
        y = torch.from_numpy(np.random.default_rng(500 + rank).standard_normal(n).astype(np.float32)).cuda()
        resid = torch.from_numpy(np.random.default_rng(9).standard_normal(n).astype(np.float32)).cuda()
        assert lib.mi355_comm_all_reduce_residual(comm.handle, y.data_ptr(), resid.data_ptr(), n, st) == 0
        torch.cuda.synchronize()
        out[("wire1",)] = resid.cpu().numpy()
    q.put((rank, out, lib.mi355_comm_p2p_error(comm.handle)))
    dist.barrier()
    comm.close()
    dist.destroy_process_group()


def test_one_shot_peer_all_reduce_two_processes_one_gpu(lib):
    """The <= 256 KiB all-reduce of the decode step as ONE kernel per rank over IPC-opened peer regions (the transport
    distributed.rs:547-654 runs as a ring): sums in rank order (bit-identical on both ranks), every size class, repeated
    calls, hipGraph replay, and the reference's bf16 wire numerics (attention.rs:1003-1008) bit for bit."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_p2p_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(2):
        r = q.get(timeout=300)
        res[r[0]] = r[1:]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert res[0][1] == 0 and res[1][1] == 0
    for n in (100, 4096, 5000, 16384, 65536):
        for it in range(4):
            a = np.random.default_rng(1000 * n + 10 * it + 0).standard_normal(n).astype(np.float32)
            b = np.random.default_rng(1000 * n + 10 * it + 1).standard_normal(n).astype(np.float32)
            want = a + b                                        # f32 add in rank order
            for rank in (0, 1):
                assert np.array_equal(res[rank][0][("sum", n, it)], want), (n, it, rank)
    for it in range(3):
        want = np.random.default_rng(77 + 10 * it).standard_normal(4096).astype(np.float32) + \
               np.random.default_rng(77 + 10 * it + 1).standard_normal(4096).astype(np.float32)
        for rank in (0, 1):
            assert np.array_equal(res[rank][0][("graph", it)], want), (it, rank)
    y0 = np.random.default_rng(500).standard_normal(8192).astype(np.float32)
    y1 = np.random.default_rng(501).standard_normal(8192).astype(np.float32)
    resid = np.random.default_rng(9).standard_normal(8192).astype(np.float32)
    want = resid + O.round_bf16(O.round_bf16(y0) + O.round_bf16(y1))
    for rank in (0, 1):
        assert np.array_equal(res[rank][0][("wire1",)], want), rank


@pytest.mark.timeout(900)
def test_bench_py_gpus_2_rehearsed_on_one_device():
    """the command the driver runs for the scaling record -- `python bench.py --gpus 2 ...` -- rehearsed on THIS box with
    both ranks on cuda:0 (`--same-device`; the line is marked invalid): bench.py spawns its ranks (communicator.rs:704-785), the REAL model is
    sharded (model.py load_synthetic: every rank keeps its shard of the same global tensors; distributed.rs:243-249,696-765), the ranks agree
    on the transport (RCCL refuses two ranks on one GPU -> the one-shot peer kernel over IPC for the all-reduces C1 / C2 behind its
    self-test, host-staged vocabulary gather C3), run the settle / blocks / roofline sequence with a collective inside every step, and rank 0
    prints ONE line.  Then the same with the device communicator FORCED to fail on rank 1 (MI355_BENCH_FAIL_COMM_RANK): every rank takes the
    gloo fallback together.  Both sharded runs produce the greedy tokens of the unsharded run of the same synthetic model."""
    import json
    import subprocess
    import sys
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--full", "--layers", "2", "--steps", "6", "--warmup", "2", "--no-batch32", "--no-cpu-baseline", "--parity", "off", "--legs", "none",
              "--settle-steps", "6"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "MI355_BENCH_FAIL_COMM_RANK")}
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")

    def run(extra, **envx):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + extra + common, env=dict(env, **envx), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=420, cwd=root)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        return json.loads(lines[0])
    one = run(["--gpus", "1"])
    assert one["n_gpus"] == 1 and len(one["config"]["first_tokens"]) == 8
    two = run(["--gpus", "2", "--same-device"])
    assert two["n_gpus"] == 2 and two["config"]["ranks"] == 2 and two["config"]["parallelism"] == "tp2" and two["config"]["same_device"] is True
    assert "ONE device" in two["invalid"] and two["scaling"] == "strong"
    assert two["config"]["all_reduce"].startswith("FALLBACK: one-shot peer kernel over IPC"), two["config"]["all_reduce"]
    assert "RCCL refuses duplicate GPUs" in two["config"]["all_reduce"]
    assert two["config"]["graph"] is False                     # host-staged vocabulary gather: eager steps
    assert two["config"]["first_tokens"] == one["config"]["first_tokens"], (one["config"]["first_tokens"], two["config"]["first_tokens"])
    assert two["value"] > 0 and two["config"]["timing"]["eager_steps_in_timed_region"] == 3 * 8
    forced = run(["--gpus", "2", "--same-device"], MI355_BENCH_FAIL_COMM_RANK="1")
    assert forced["n_gpus"] == 2 and forced["config"]["ranks"] == 2
    assert forced["config"]["all_reduce"].startswith("FALLBACK: host-staged collectives over gloo"), forced["config"]["all_reduce"]
    assert "forced failure" in forced["config"]["all_reduce"] and "rank 1" in forced["config"]["all_reduce"]
    assert forced["config"]["first_tokens"] == one["config"]["first_tokens"]
