"""CPU: the n-gram LM inside the CTC prefix beam search (ob_ctc_beam_search_lm, csrc/beam.hip):
the oracle of tests/ctc_beam_lm_ref.py against an answer derived by hand, the new symbols, the
workspace call's limits, the two new keywords of encode_and_decode / GraphedInference and their
ValueErrors. The search itself runs on the device (tests/test_beam_lm_gpu.py)."""
import inspect
import math

import numpy as np
import pytest

from ctc_beam_lm_ref import fuse, lm_beam_search
from ctc_beam_ref import beam_search
from ngram_ref import RefLM

BLANK = 3


def test_known_answer_by_hand():
    """T = 2, V = 5, beam 2, every token a candidate, a 3-entry bigram table, lm_weight 1; logits,
    table values and weights are binary fractions. P1, P2 are the frames' softmax rows (about
    1/2, 1/16, 1/16, 1/8, 1/4 and 1/4, 1/16, 1/16, 1/2, 1/8 for tokens 0, 1, 2, blank, 4).

    LM: (0,) = (-8, -0.5), (4,) = (-0.5, 0), (1, 4) = (-0.25, 0), unk = -16. So
    score([bos], 4) = -0.25 (the bigram), score([bos], 0) = -8 (no bigram, [bos] is no entry, the
    unigram), score([bos], 1) = score([bos], 2) = -16, score([bos, 4], 0) = 0 - 8,
    score([bos, 4], eos) = 0 - 16, score([bos], eos) = -16.

    Frame 1 keys: () ln P1[3] ~ -2.1; (0) ln P1[0] - 8 ~ -8.7; (4) ln P1[4] - 0.25 ~ -1.6; (1), (2)
    ~ -18.8. The beam keeps [(4), ()]; the search without the LM keeps [(0), (4)] and drops ().
    Frame 2 from (4) (p_b 0, p_nb P1[4]): (4).p_b = P1[4] P2[3]; the repeat adds p_b = 0; (4, 0),
    (4, 1), (4, 2) are new. From () (p_b P1[3]): ().p_b = P1[3] P2[3]; (0), (1), (2) are new; the
    extension by 4 lands on the live (4): (4).p_nb = P1[3] P2[4], a merge. Keys: (4)
    ln(P1[4] P2[3] + P1[3] P2[4]) - 0.25 ~ -2.2; () ~ -2.8; (4, 0) ~ -2.8 - 8.25; the rest lower.
    The beam keeps [(4), ()]. Totals: (4) ctc - 16.25, () ctc - 16: ~ -18.2 and ~ -18.8.
    Without the LM the best prefix is (0)."""
    x = np.array([[-0.75, -2.75, -2.75, -2.125, -1.375],
                  [-1.375, -2.75, -2.75, -0.75, -2.125]], np.float32)
    P = np.exp(x.astype(np.float64))
    P /= P.sum(axis=1, keepdims=True)
    lm = RefLM({(0,): (-8.0, -0.5), (4,): (-0.5, 0.0), (1, 4): (-0.25, 0.0)}, 2, unk_logp=-16.0)
    assert beam_search(x, 2, BLANK, 20).tokens == [0]
    res = lm_beam_search(x, lm, 1.0, 0.0, beam=2, blank=BLANK, top_k=20)
    assert res.final_beam == [[4], []] and res.merges == 1
    ctc4 = math.log(P[0, 4] * P[1, 3] + P[0, 3] * P[1, 4])
    ctc0 = math.log(P[0, 3] * P[1, 3])
    (_, c_a, l_a, t_a), (_, c_b, l_b, t_b) = res.beam
    assert abs(c_a - ctc4) <= 1e-12 and abs(c_b - ctc0) <= 1e-12
    assert (l_a, l_b) == (-16.25, -16.0)                  # binary fractions: exact
    assert t_a == c_a + l_a and t_b == c_b + l_b
    assert abs(res.gap - ((ctc4 - 16.25) - (ctc0 - 16.0))) <= 1e-12 and res.margin == res.gap
    # the insertion bonus: the same survivors, 0.5 per token on the totals
    bon = lm_beam_search(x, lm, 1.0, 0.5, beam=2, blank=BLANK, top_k=20)
    assert bon.final_beam == [[4], []]
    assert bon.beam[0][3] == (c_a + l_a) + 0.5 and bon.beam[1][3] == t_b
    # the weight 0 and bonus 0: the plain search, its order and scores
    plain = lm_beam_search(x, lm, 0.0, 0.0, beam=2, blank=BLANK, top_k=20)
    assert plain.final_beam == beam_search(x, 2, BLANK, 20).final_beam
    assert plain.beam[0][1] == beam_search(x, 2, BLANK, 20).score
    assert fuse(1.0, 0.5, -3.0, 0.25, 2) == 0.0


def test_symbols_are_exported_with_signatures():
    import ctypes

    import onebit_asr
    from onebit_asr import _lib, infer

    lib = _lib.load()
    for name, nargs in (("ob_ctc_beam_search_lm_workspace", 6), ("ob_ctc_beam_search_lm", 27)):
        res, args = _lib.SIGNATURES[name]
        assert len(args) == nargs and getattr(lib, name).argtypes == args
    assert _lib.SIGNATURES["ob_ctc_beam_search_lm_workspace"][0] is ctypes.c_size_t
    assert lib.ob_abi_version() == 4                                # entries were only added
    assert onebit_asr.ctc_beam_search_lm_device is infer.ctc_beam_search_lm_device
    assert "ctc_beam_search_lm_device" in infer.__all__
    p = inspect.signature(infer.ctc_beam_search_lm_device).parameters
    assert list(p) == ["logits", "lens", "lm", "lm_weight", "ins_bonus", "beam_size", "nbest",
                       "blank_id", "top_k_per_t"]
    assert (p["ins_bonus"].default, p["beam_size"].default, p["nbest"].default,
            p["blank_id"].default, p["top_k_per_t"].default) == (0.0, 10, None, 3, 20)


def test_workspace_limits_and_argument_validation():
    from onebit_asr import _lib

    lib = _lib.load()
    ws = lib.ob_ctc_beam_search_lm_workspace
    assert ws(32, 249, 5004, 10, 20, 4) == lib.ob_ctc_beam_search_nbest_workspace(32, 249, 5004,
                                                                                   10, 20) > 0
    assert ws(2, 16, 65535, 32, 64, 1) > 0
    assert ws(2, 16, 5004, 10, 20, 5) == 0 and ws(2, 16, 5004, 10, 20, 0) == 0      # order
    assert ws(2, 16, 65536, 10, 20, 4) == 0                                         # V
    assert ws(2, 16, 5004, 33, 20, 4) == 0 and ws(2, 16, 5004, 10, 65, 4) == 0      # beam, top_k
    f = 0x1000
    NULL, SHAPE, WORKSPACE, ALIGN = -1, -2, -4, -5

    def call(**kw):
        a = dict(logits=f, lens=f, B=2, T=16, V=40, blank=3, beam=10, top_k=20, nbest=10, table=f,
                 slots=64, max_probe=4, order=3, unk=-23.0, bos=1, eos=2, lw=0.5, bonus=0.0, ws=f,
                 ws_bytes=1 << 30, hyp=f, hyp_len=f, n_hyp=f, ctc=f, lm=f, total=f)
        a.update(kw)
        return lib.ob_ctc_beam_search_lm(*a.values(), None)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(order=5), dict(V=65536), dict(beam=33, nbest=33), dict(top_k=65),
               dict(nbest=11), dict(nbest=0), dict(blank=40), dict(bos=40), dict(eos=-1),
               dict(slots=48), dict(max_probe=65), dict(lw=-0.5), dict(lw=nan), dict(lw=inf),
               dict(bonus=nan), dict(bonus=-inf), dict(unk=-inf)):
        assert call(**kw) == SHAPE, kw
    for name in ("logits", "lens", "table", "ws", "hyp", "hyp_len", "n_hyp", "ctc", "lm", "total"):
        assert call(**{name: None}) == NULL, name
    for name in ("lens", "ws", "ctc", "lm", "total"):                               # 8-byte
        assert call(**{name: 0x3004}) == ALIGN, name
    for name in ("logits", "hyp", "hyp_len", "n_hyp"):
        assert call(**{name: 0x3002}) == ALIGN, name
    assert call(table=0x3008) == ALIGN                                              # 16-byte
    assert call(ws_bytes=8) == WORKSPACE
    assert call(B=0, logits=None, lens=None, hyp=None, ctc=None) == 0               # no launch


def test_fusion_keywords_are_pinned():
    from onebit_asr.infer import LM_FUSIONS, GraphedInference, encode_and_decode

    assert LM_FUSIONS == ("rescore", "first_pass")
    for fn in (encode_and_decode, GraphedInference.__init__):
        p = inspect.signature(fn).parameters
        names = list(p)
        assert names[-4:] == ["lm_fusion", "ins_bonus", "joint_ctc_weight", "ctc_cand"]
        assert names.index("lm_weight") + 1 == names.index("lm_fusion")
        assert p["lm_fusion"].default == "rescore" and p["ins_bonus"].default == 0.0
        assert p["lm_fusion"].kind is p["ins_bonus"].kind is inspect.Parameter.KEYWORD_ONLY


def test_fusion_value_errors():
    import torch

    from onebit_asr.infer import GraphedInference, ctc_beam_search_lm_device, encode_and_decode

    class FakeLM:            # the checks run ahead of the forward: nothing of the LM is touched
        bos, eos, order = 1, 2, 3

    lm = FakeLM()

    def both(match, **kw):
        with pytest.raises(ValueError, match=match):
            encode_and_decode(None, {}, **kw)
        with pytest.raises(ValueError, match=match):
            GraphedInference(torch.nn.Identity(), act_quant=None, **kw)
    for dec in ("greedy", "rescore", "attention"):
        both("first_pass", decoder=dec, lm=lm, lm_weight=0.0 if dec == "greedy" else 0.5,
             lm_fusion="first_pass")
    both("first_pass", decoder="beam", lm_fusion="first_pass")                   # no LM
    both("first_pass", decoder="beam", lm=lm, lm_weight=0.0, lm_fusion="first_pass")
    both("lm_fusion", decoder="beam", lm=lm, lm_weight=0.5, lm_fusion="second_pass")
    both("lm_fusion", decoder="greedy", lm_fusion="fused")
    for w in (-0.5, float("nan")):
        both("lm_weight", decoder="beam", lm=lm, lm_weight=w, lm_fusion="first_pass")
    for bonus in (float("nan"), float("inf")):
        both("ins_bonus", decoder="beam", lm=lm, lm_weight=0.5, lm_fusion="first_pass",
             ins_bonus=bonus)
    both("ins_bonus", decoder="beam", lm=lm, lm_weight=0.5, ins_bonus=0.5)       # re-ranking
    gi = GraphedInference(torch.nn.Identity(), act_quant=None, decoder="beam", lm=lm,
                          lm_weight=0.5, lm_fusion="first_pass", ins_bonus=0.25)
    assert (gi.lm_fusion, gi.ins_bonus, gi.use_lm) == ("first_pass", 0.25, True)
    z = torch.zeros(2, 9, 40)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc_beam_search_lm_device(z, torch.tensor([9, 3]), lm, 0.5)
