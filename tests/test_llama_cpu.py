"""The Llama decoder without a GPU: tests/llama_ref.py (the statement the GPU tests hold the library to) against the reference's own
``LlamaDecoder`` through tests/golden/llama_ref.npz (tools/make_llama_golden.py), and every refusal that is decided on the host."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import llama_ref as R
from audiocodecs_amd import _native, llama
from audiocodecs_amd.llama import LLAMA_TINY, LLAMA_TTS, LlamaConfig, LlamaDecoder
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "llama_ref.npz")


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return g, json.loads(bytes(g["meta_json"]).decode())


@pytest.fixture(scope="module")
def stated(golden):
    """name -> (the fp64 and the fp32 statement's full logits, cached-step logits, and the fp64 greedy run) -- computed once."""
    g, meta = golden
    out = {}
    for name, cfg in R.CONFIGS.items():
        c = meta["cases"][name]
        toks = torch.from_numpy(g[f"{name}_toks"].astype(np.int64))
        prompt = torch.from_numpy(g[f"{name}_prompt"]) if c["P"] else None
        res = {}
        for dtype in (torch.float64, torch.float32):
            s = R.Statement(cfg, R.weights(cfg), dtype)
            embs = s.embed(toks, prompt)
            full = s.forward(embs)
            s.reset()
            n0 = embs.shape[1] - meta["steps"]
            s.forward(embs[:, :n0])
            cached = torch.cat([s.forward(embs[:, i:i + 1]) for i in range(n0, embs.shape[1])], dim=1)
            res[dtype] = (full, cached)
        s64 = R.Statement(cfg, R.weights(cfg), torch.float64)
        res["greedy"] = s64.generate_greedy(toks[:, :1], c["eos_id"], prompt, meta["gen"])
        res["free"] = s64.generate_greedy(toks[:, :1], -1, prompt, meta["gen"])
        out[name] = res
    return out


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_inputs_are_the_generated_ones(golden, name):
    g, meta = golden
    toks, prompt = R.inputs(R.CONFIGS[name], meta["B"], meta["cases"][name]["P"], meta["T"])
    assert np.array_equal(g[f"{name}_toks"], toks.numpy())
    if prompt is not None:
        assert np.array_equal(g[f"{name}_prompt"], prompt.numpy())


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_statement_matches_the_reference_logits(golden, stated, name):
    g, _ = golden
    for i, key in enumerate(("full", "cached")):
        gold = torch.from_numpy(g[f"{name}_{key}"])
        s64, s32 = stated[name][torch.float64][i], stated[name][torch.float32][i]
        bound = R.K_BOUND * R.err(s32, s64)
        e = R.err(gold, s64)
        print(f"{name} {key}: |fp64 - golden| = {e:.3g}, bound {bound:.3g}")
        assert gold.shape == s64.shape and bound > 0.0
        assert e <= bound, (key, e, bound)


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_statement_greedy_tokens_match_the_reference(golden, stated, name):
    g, meta = golden
    c = meta["cases"][name]
    err32 = R.err(stated[name][torch.float32][0], stated[name][torch.float64][0])
    for key, eos in (("hyp", c["eos_id"]), ("free", -1)):
        rows, log = stated[name]["greedy" if key == "hyp" else "free"]
        gold = g[f"{name}_{key}"].astype(np.int64)
        gap = R.top2_gap(log)                                   # [steps, B]
        skipped = total = 0
        for i, row in enumerate(rows):
            want = gold[i][gold[i] >= 0] if key == "hyp" else gold[i]
            n = min(len(row), len(want))
            sure = (gap[:n, i] > R.GAP_FACTOR * err32).numpy()
            total += n
            skipped += int((~sure).sum())
            assert np.array_equal(row.numpy()[:n][sure], want[:n][sure]), (key, i)
            if sure.all():
                assert len(row) == len(want), (key, i)
        print(f"{name} {key}: smallest gap {float(gap.min()):.3g}, error {err32:.3g}, {skipped} of {total} steps skipped")
        assert skipped <= 0.03 * total
    assert c["lens"] == [int((g[f"{name}_hyp"][i] >= 0).sum()) for i in range(meta["B"])] and min(c["lens"]) < meta["gen"]


def test_wrong_grouping_is_a_different_statement():
    cfg = R.TINY_G2
    toks, _ = R.inputs(cfg, 3, 0, 21)
    a, b = R.Statement(cfg, R.weights(cfg)), R.Statement(cfg, R.weights(cfg), wrong_grouping=True)
    assert R.err(a.forward(a.embed(toks)), b.forward(b.embed(toks))) > 1e-2


def test_rope_table_is_the_references():
    cos, sin = llama.rope_table(R.TINY_HD128)
    assert cos.shape == (1024, 64) and cos.dtype == torch.float32
    assert float(cos[0].min()) == 1.0 and float(sin[0].abs().max()) == 0.0
    # fp32 angles: at position 1000 they differ from the fp64 ones by far more than one fp32 rounding of the cosine
    inv = 1.0 / (10000.0 ** (torch.arange(0, 128, 2).double() / 128))
    assert float((cos[1000].double() - torch.cos(1000 * inv)).abs().max()) > 1e-6


def test_create_refuses_without_gpu():
    L = _native.lib()
    h = C.c_void_p()
    assert L.ac_lm_create(C.byref(_native.AcLmConfig()), C.byref(h)) == -1       # struct_size == 0
    assert L.ac_lm_create(None, C.byref(h)) == -1

    def rc(cfg, **raw):
        c = llama._struct(cfg)
        for k, v in raw.items():
            setattr(c, k, v)
        c.struct_size = C.sizeof(c)
        c.device = 1 << 20           # (a valid config stops at the device: never created here)
        return L.ac_lm_create(C.byref(c), C.byref(h))

    ok = rc(LLAMA_TINY)
    assert ok < -1, ok
    assert rc(LLAMA_TTS) == ok and rc(dataclasses.replace(LLAMA_TTS, prompt_dim=512)) == ok
    for cfg in R.CONFIGS.values():
        assert rc(cfg) == ok
    for bad in (dict(n_heads=3), dict(n_heads=4, n_kv_heads=3), dict(dim=20, n_heads=4), dict(n_heads=16, n_kv_heads=1), dict(ffn_dim=130),
                dict(prompt_dim=23), dict(dim=2048, n_heads=4), dict(n_layers=0), dict(num_codebooks=0), dict(norm_eps=0.0)):
        assert rc(dataclasses.replace(LLAMA_TINY, **bad)) == -1, bad
    for raw in (dict(vocab_size=1), dict(vocab_size=16385)):
        assert rc(LLAMA_TINY, **raw) == -1, raw
    assert L.ac_lm_state_bytes(None, 1, 16, 0) == 0 and L.ac_lm_workspace_bytes(None, 1, 1, 16) == 0
    assert L.ac_lm_step(None, None, 0, 1, 16, 1, 0, 1.0, 0.9, 0, None, None, 0, None) == -1


def test_python_refusals():
    sd = R.weights(R.TINY)
    dec = LlamaDecoder(state_dict=sd, config=R.TINY)
    bos = torch.zeros(2, 1, dtype=torch.int64)
    prompt = torch.zeros(2, 6, 24)
    with pytest.raises(NotImplementedError):
        dec.generate(bos, 5, prompt, eos_threshold=2.0, seed=0)
    with pytest.raises(NotImplementedError):
        dec.generate(bos, 5, prompt, use_kv_cache=False, seed=0)
    with pytest.raises(NotImplementedError):
        dec.generate(bos, 5, prompt, batch_parallel=False, seed=0)
    with pytest.raises(NotImplementedError):
        dec.forward(torch.zeros(2, 3, 64), mask=None)
    with pytest.raises(NotImplementedError):
        dec.forward(torch.zeros(2, 3, 64), mask=torch.zeros(3, 3))
    with pytest.raises(NotImplementedError):
        LlamaDecoder(state_dict=sd, config=dataclasses.replace(R.TINY, embedding_kwargs={"padding_idx": True}))
    with pytest.raises(TypeError):
        dec.generate(bos, 5, prompt)                                     # `seed` is required
    with pytest.raises(ValueError):
        dec.generate(bos, 5, prompt, seed=None)
    with pytest.raises(ValueError):
        dec.generate(bos, 5, prompt[:, :5], seed=0)                      # 5 prompt rows, 2 codebooks
    with pytest.raises(ValueError):
        dec.generate(bos, 5, prompt, max_gen_toks=2 * 512 - 6, seed=0)   # 6 + 1 + 1018 > 1024
    with pytest.raises(ValueError):
        dec.generate(torch.zeros(65, 1, dtype=torch.int64), 5, seed=0)
    with pytest.raises(ValueError):
        dec.generate(bos, 5, prompt, top_p=1.5, seed=0)
    with pytest.raises(ValueError):
        dec.generate(bos, 5, prompt, temp=0.0, seed=0)
    with pytest.raises(ValueError):
        dec.generate(bos, 5, prompt, max_gen_toks=0, seed=0)
    for vocab in (1, 16385):
        with pytest.raises(ValueError):
            LlamaDecoder(state_dict=sd, config=dataclasses.replace(R.TINY, vocab_size=vocab))
    with pytest.raises(KeyError):
        LlamaDecoder(state_dict={k: v for k, v in sd.items() if k != "layers.1.feed_forward.w3.weight"}, config=R.TINY)
    with pytest.raises(KeyError):
        LlamaDecoder(state_dict={k: v for k, v in sd.items() if k != "prompt.weight"}, config=R.TINY)
    with pytest.raises(ValueError):
        dec.embed(torch.zeros(2, 3))                                     # floating-point ids
    with pytest.raises(ValueError):
        dec.embed(bos, torch.zeros(2, 6, 25))
    with pytest.raises(ValueError):
        dec.forward(torch.zeros(2, 3, 63))
    with pytest.raises(_native.NativeError):
        dec.embed(bos)                                                   # a CPU tensor: there is no CPU fallback
    with pytest.raises(_native.NativeError):
        dec.generate(bos, 5, prompt, seed=0)


def test_names_and_stack_generated():
    import audiocodecs_amd

    for name in ("LlamaDecoder", "LlamaConfig", "LLAMA_TTS", "LLAMA_TINY", "stack_generated"):
        assert name in audiocodecs_amd.__all__ and hasattr(audiocodecs_amd, name)
    assert isinstance(LLAMA_TTS, LlamaConfig) and (LLAMA_TTS.n_layers, LLAMA_TTS.dim, LLAMA_TTS.n_heads, LLAMA_TTS.n_kv_heads, LLAMA_TTS.head_dim) == (12, 512, 4, 1, 128)
    assert (LLAMA_TTS.ffn, LLAMA_TTS.vocab_size, LLAMA_TTS.num_codebooks, LLAMA_TTS.max_seq_len, LLAMA_TTS.prompt_dim) == (2048, 1026, 2, 8192, None)
    hyp = [torch.tensor([1, 2, 3, 1025]), torch.tensor([7, 1024, 9, 10])]
    out = audiocodecs_amd.stack_generated(hyp, 2, 1024)
    assert out.tolist() == [[[1, 2], [3, 1023]], [[7, 1023], [9, 10]]]
    with pytest.raises(RuntimeError):
        audiocodecs_amd.stack_generated([hyp[0], hyp[1][:2]], 2, 1024)      # rows of different lengths do not stack
