"""CPU: the oracle of the joint CTC/attention beam search (tests/joint_ref.py) against a
brute-force enumeration of every alignment and against answers derived by hand
(tests/golden/joint_kat.json); its w = 0 search against ``attdec_ref.beam_search``; the argument
checks of the new C entry points, which fail before any HIP call; the Python surface.

Figures seen (-s): recursion against enumeration, worst difference 3.6e-15 over the five shapes
(every prefix of up to 4 tokens), -inf exactly where no alignment exists.
"""
import itertools
import json
import math
from pathlib import Path

import numpy as np
import pytest

import attdec_ref as ar
import joint_ref as jr

NEG_INF = -math.inf
KAT = json.loads((Path(__file__).parent / "golden" / "joint_kat.json").read_text())


@pytest.mark.parametrize("T,V", [(1, 3), (2, 3), (4, 4), (5, 3), (6, 3)])
def test_recursion_matches_enumeration(T, V):
    blank = V - 1
    rng = np.random.default_rng(100 * T + V)
    x = jr.log_softmax64(rng.standard_normal((T, V)).astype(np.float32) * 2.0)
    worst, n_inf = 0.0, 0
    for n in range(5):
        for g in itertools.product(range(V - 1), repeat=n):
            gn, gb, psi = jr.prefix_state(x, blank, g)
            want_psi, want_full = jr.brute_force(x, blank, g)
            for got, want in ((psi, want_psi), (jr.eos_score(gn, gb), want_full)):
                assert not math.isnan(got)
                if want == NEG_INF:
                    n_inf += 1
                    assert got == NEG_INF, (g, got)
                else:
                    worst = max(worst, abs(got - want))
    print(f"T={T} V={V}: worst {worst:.2e}, {n_inf} impossible")
    assert worst <= 1e-12
    if (T, V) == (4, 4):
        assert jr.prefix_state(x, blank, [0, 0, 0])[2] == NEG_INF   # needs 5 frames


def test_known_answers_by_hand():
    assert KAT["V"] == 4 and KAT["blank"] == 3
    for c in KAT["cases"]:
        x = np.full((c["T"], 4), math.log(0.25))
        gn, gb, psi = jr.prefix_state(x, 3, c["prefix"])
        got = psi if c["kind"] == "psi" else jr.eos_score(gn, gb)
        if c["num"] == 0:
            assert got == NEG_INF, c
        else:
            assert abs(got - math.log(c["num"] / c["den"])) <= 1e-14, (c, got)


@pytest.mark.parametrize("N,alpha", [(1, 0.0), (4, 0.0), (10, 0.6)])
def test_weight_zero_is_the_attention_search(N, alpha):
    V, L = 12, 6
    x = jr.log_softmax64(np.random.default_rng(3).standard_normal((5, V)).astype(np.float32))
    for u in range(3):
        logp = jr.hash_logp(100 * N + u, V, 2)
        ref = ar.beam_search(logp, N, L, alpha)
        got = jr.joint_search(logp, x, N, N, L, 0.0, alpha)
        assert got.hyps == ref.hyps and got.scores == ref.scores == got.att
        assert got.finished == ref.finished and got.trace == ref.trace and got.dropped == 0


def test_joint_oracle_drops_and_can_end_empty():
    """T = 1: after one token every extension but eos is CTC-impossible; when eos is outside a
    row's K candidates the utterance ends without a hypothesis."""
    V = 12
    x = jr.log_softmax64(np.random.default_rng(4).standard_normal((1, V)).astype(np.float32))
    lp = -np.arange(V, dtype=np.float64)        # eos (id 2) is the best candidate
    res = jr.joint_search(lambda ps: [lp for _ in ps], x, 2, 4, 3, 0.5)
    assert all(res.finished) and res.dropped > 0 and all(len(h) <= 1 for h in res.hyps)
    lp2 = np.arange(V, dtype=np.float64) - V    # eos is among the worst: never in the top 4
    res = jr.joint_search(lambda ps: [lp2 for _ in ps], x, 2, 4, 3, 0.5)
    assert res.hyps == [] and all(v == ar.DEAD for _, v, _ in res.trace[-1])
    assert all(s == NEG_INF for _, _, s in res.trace[-1])


def test_argument_validation_without_a_device():
    from onebit_asr import _lib

    lib = _lib.load()
    f, g = 0x1000, 0x2000
    NULL, SHAPE, ALIGN = -1, -2, -5
    sup = lib.ob_ctc_prefix_supported
    assert sup(10, 20, 249) and sup(1, 1, 1) and sup(32, 32, 256)
    assert not sup(10, 9, 249) and not sup(10, 33, 249) and not sup(0, 4, 9)      # K < N, K = 33
    assert not sup(10, 20, 257) and not sup(10, 20, 0)                            # T'
    ws = lib.ob_ctc_prefix_workspace
    assert ws(256, 10, 10, 249) == ws(256, 10, 32, 249) == 2 * 2560 * 249 * 2 * 8  # not K's
    assert ws(256, 10, 9, 249) == 0 and ws(256, 10, 33, 249) == 0 and ws(256, 10, 20, 257) == 0
    print(f"state workspace at B=256 N=10 T'=249: {ws(256, 10, 20, 249)} bytes for any K")
    # frame lse: logits, lens, B, T', V, flse
    fl = lib.ob_ctc_frame_lse
    assert fl(f, f, 2, 257, 9, f, None) == SHAPE and fl(f, f, 2, 0, 9, f, None) == SHAPE
    assert fl(f, f, 2, 7, 0, f, None) == SHAPE
    assert fl(None, f, 2, 7, 9, f, None) == NULL and fl(f, None, 2, 7, 9, f, None) == NULL
    assert fl(f, f, 2, 7, 9, None, None) == NULL
    assert fl(f, f, 2, 7, 9, 0x1004, None) == ALIGN and fl(f, 0x1004, 2, 7, 9, f, None) == ALIGN
    assert fl(0x1002, f, 2, 7, 9, f, None) == ALIGN
    assert fl(None, None, 0, 7, 9, None, None) == 0                               # B == 0
    # scorer step: logits, flse, lens, topi, tok, len, link, skip, B, N, K, T', V, blank, eos,
    #              state_in, state_out, cpsi
    ps = lib.ob_ctc_prefix_step

    def call(a=None, **kw):
        args = dict(logits=f, flse=f, lens=f, topi=f, tok=f, len=f, link=f, skip=f, B=2, N=4, K=8,
                    Tp=7, V=9, blank=3, eos=2, sin=f, sout=g, cpsi=f)
        args.update(kw)
        return ps(*args.values(), None)
    assert call(K=3) == SHAPE and call(K=33) == SHAPE and call(Tp=257) == SHAPE
    assert call(N=0) == SHAPE and call(blank=9) == SHAPE and call(eos=-1) == SHAPE
    assert call(sout=f) == SHAPE                                                  # in == out
    for name in ("logits", "flse", "lens", "topi", "tok", "len", "link", "skip", "sin", "sout",
                 "cpsi"):
        assert call(**{name: None}) == NULL, name
    for name in ("flse", "lens", "tok", "sin", "sout", "cpsi"):                   # 8-byte
        assert call(**{name: 0x3004}) == ALIGN, name
    for name in ("logits", "topi", "len", "link"):
        assert call(**{name: 0x3002}) == ALIGN, name
    assert ps(*([None] * 8), 0, 4, 8, 7, 9, 3, 2, None, None, None, None) == 0    # B == 0
    # joint step: lse, topv, topi, cpsi, w, B, N, K, L, t, eos, pad, norm, anc_in, anc_out, score,
    #             att, ctc, len, fin, tok, skip, link, trace_parent, trace_token, trace_score
    js = lib.ob_attdec_joint_step

    def jcall(**kw):
        args = dict(lse=f, topv=f, topi=f, cpsi=f, w=0.3, B=2, N=4, K=8, L=12, t=0, eos=2, pad=0,
                    norm=f, anc_in=f, anc_out=g, score=f, att=f, ctc=f, len=f, fin=f, tok=f,
                    skip=f, link=f, trp=f, trt=f, trs=f)
        args.update(kw)
        return js(*args.values(), None)
    assert jcall(K=3) == SHAPE and jcall(K=33) == SHAPE and jcall(N=33, K=33) == SHAPE
    assert jcall(t=12) == SHAPE and jcall(L=256) == SHAPE and jcall(anc_out=f) == SHAPE
    assert jcall(w=-0.1) == SHAPE and jcall(w=1.5) == SHAPE and jcall(w=float("nan")) == SHAPE
    for name in ("lse", "topv", "topi", "cpsi", "norm", "anc_in", "anc_out", "score", "att", "ctc",
                 "len", "fin", "tok", "skip", "link", "trp", "trt", "trs"):
        assert jcall(**{name: None}) == NULL, name
    for name in ("lse", "cpsi", "norm", "score", "att", "ctc", "tok", "trs"):     # 8-byte
        assert jcall(**{name: 0x3004}) == ALIGN, name
    for name in ("topv", "topi", "anc_in", "len", "link", "trp", "trt"):
        assert jcall(**{name: 0x3002}) == ALIGN, name
    assert jcall(B=0, **{k: None for k in ("lse", "topv", "topi", "cpsi", "norm", "anc_in",
                                           "anc_out", "score", "att", "ctc")}) == 0


def test_decoder_switch_and_joint_keywords():
    import inspect

    import torch

    from onebit_asr.infer import DECODERS, GraphedInference, encode_and_decode

    assert DECODERS == ("greedy", "beam", "rescore", "attention")
    for fn in (encode_and_decode, GraphedInference.__init__):
        assert list(inspect.signature(fn).parameters)[-2:] == ["joint_ctc_weight", "ctc_cand"]
        p = inspect.signature(fn).parameters
        assert p["joint_ctc_weight"].default == 0.0 and p["ctc_cand"].default is None
    for dec in ("greedy", "beam", "rescore"):
        with pytest.raises(ValueError, match="joint_ctc_weight"):
            encode_and_decode(None, {}, decoder=dec, joint_ctc_weight=0.3)
        with pytest.raises(ValueError, match="joint_ctc_weight"):
            GraphedInference(torch.nn.Identity(), act_quant=None, decoder=dec,
                             joint_ctc_weight=0.3)
    for w in (-0.1, 1.5):
        with pytest.raises(ValueError, match="joint_ctc_weight"):
            encode_and_decode(None, {}, decoder="attention", joint_ctc_weight=w)
        with pytest.raises(ValueError, match="joint_ctc_weight"):
            GraphedInference(torch.nn.Identity(), act_quant=None, decoder="attention",
                             joint_ctc_weight=w)
    gi = GraphedInference(torch.nn.Identity(), act_quant=None, decoder="attention", beam_size=4,
                          max_len=12, joint_ctc_weight=0.3, ctc_cand=8)
    assert (gi.joint_ctc_weight, gi.ctc_cand) == (0.3, 8)


def test_python_surface_on_cpu():
    import torch

    import onebit_asr
    from onebit_asr.attdec import ctc_frame_lse, ctc_prefix_step, joint_beam_search
    from onebit_asr.conformer import ConformerASR
    from onebit_asr.data import CFG1, synthetic_batch
    from onebit_asr.infer import encode_and_decode

    assert onebit_asr.joint_beam_search is joint_beam_search
    assert callable(onebit_asr.joint_decode_batch)
    torch.manual_seed(0)
    model = ConformerASR(80, 40, **CFG1).eval()
    enc, mask = torch.zeros(2, 9, 64), torch.ones(2, 9, dtype=torch.long)
    z = torch.zeros(2, 9, 40)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        joint_beam_search(model, enc, mask, z, beam_size=4, max_len=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        onebit_asr.joint_decode_batch(model, enc, mask, z, beam_size=4, max_len=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc_frame_lse(z, torch.tensor([9, 3]))
    i32 = torch.int32
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc_prefix_step(z, torch.zeros(2, 9, dtype=torch.float64), torch.tensor([9, 3]),
                        torch.zeros(2, 4, dtype=i32), torch.zeros(2, dtype=torch.int64),
                        torch.zeros(2, dtype=i32), torch.zeros(2, 2, dtype=i32),
                        torch.zeros(2, dtype=torch.uint8), torch.zeros(2, 9, 2, dtype=torch.float64),
                        torch.zeros(2, 9, 2, dtype=torch.float64),
                        torch.zeros(2, 4, dtype=torch.float64))
    batch = synthetic_batch([61], [3], vocab=40, device="cpu")
    with pytest.raises(RuntimeError, match="joint_beam_search runs on the HIP library"):
        encode_and_decode(model, batch, precision=32, decoder="attention", beam_size=2, max_len=4,
                          joint_ctc_weight=0.3)


def test_search_mode_rule():
    """The one loop's mode rule (attdec._search_mode): the step entry, K, which scorers run and
    which keys info gains, for every kind of call the two public searches make."""
    from onebit_asr.attdec import _search_mode

    lm = object()                                   # (the rule only asks whether there is one)
    base, joint, fused = "ob_attdec_beam_step", "ob_attdec_joint_step", "ob_attdec_fused_step"
    # attention_beam_search: K = N, no scorer, the four base keys
    assert tuple(_search_mode(4, None, False)) == (base, 4, False, False, ())
    assert tuple(_search_mode(10, None, False)) == (base, 10, False, False, ())
    # joint_beam_search: (w, lm, lm_weight) -> entry, CTC scorer, LM scorer, info's extra keys
    cases = [((0.0, None, 0.0), (base, False, False, ("att", "ctc"))),
             ((0.3, None, 0.0), (joint, True, False, ("att", "ctc"))),
             ((1.0, None, 0.0), (joint, True, False, ("att", "ctc"))),
             ((0.0, lm, 0.0), (base, False, False, ("att", "ctc"))),      # lm_weight 0: no LM
             ((0.3, lm, 0.0), (joint, True, False, ("att", "ctc"))),
             ((0.3, None, 0.7), (joint, True, False, ("att", "ctc"))),    # a weight without an LM
             ((0.0, lm, 0.7), (fused, False, True, ("att", "ctc", "lm"))),
             ((0.3, lm, 0.7), (fused, True, True, ("att", "ctc", "lm")))]
    for (w, m, lw), (entry, ctc, lms, keys) in cases:
        got = _search_mode(4, 8, True, w, m, lw)
        assert (got.entry, got.k, got.ctc, got.lm, got.info) == (entry, 8, ctc, lms, keys), (w, lw)
        # K defaults to min(32, 2 N), whatever the mode
        assert _search_mode(4, None, True, w, m, lw) == got._replace(k=8)
        assert _search_mode(10, None, True, w, m, lw).k == 20
        assert _search_mode(20, None, True, w, m, lw).k == 32
