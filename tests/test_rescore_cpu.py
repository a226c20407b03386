"""CPU: the oracle of two-pass decoding (tests/rescore_ref.py) against answers derived by hand
and against ``ctc_beam_ref``; the argument checks of the new C entry points that fail before
any HIP call; the Python surface's decoder switch."""
import math

import numpy as np
import pytest

import rescore_ref as rr
from ctc_beam_ref import beam_search, ctc_like_logits, ragged_lens

INF = math.inf


def test_prepare_by_hand():
    # N = 3 slots, Lc = 2. Utterance 0: the empty hypothesis, one of length Lc, one absent.
    # Utterance 1: a hypothesis of length Lc + 1 -> ok = 0, every row of it as if absent.
    hyps = [[[], [7, 9]], [[5], [4, 6, 8]]]
    inp, tgt, pad, ok = rr.prepare(hyps, 3, 2)
    assert ok == [1, 0]
    assert inp[0] == [1, 0, 0] and tgt[0] == [2, -1, -1] and pad[0] == [0, 1, 1]    # [] -> [eos]
    assert inp[1] == [1, 7, 9] and tgt[1] == [7, 9, 2] and pad[1] == [0, 0, 0]      # length Lc
    assert inp[2] == [1, 0, 0] and tgt[2] == [-1, -1, -1] and pad[2] == [0, 1, 1]   # absent
    for r in (3, 4, 5):                                                              # ok = 0
        assert inp[r] == [1, 0, 0] and tgt[r] == [-1, -1, -1] and pad[r] == [0, 1, 1]
    # Lc = 3 takes the long one: bos y1 y2 y3 / y1 y2 y3 eos
    inp, tgt, pad, ok = rr.prepare(hyps, 3, 3)
    assert ok == [1, 1]
    assert inp[4] == [1, 4, 6, 8] and tgt[4] == [4, 6, 8, 2] and pad[4] == [0, 0, 0, 0]
    assert inp[3] == [1, 5, 0, 0] and tgt[3] == [5, 2, -1, -1] and pad[3] == [0, 0, 1, 1]
    # no row is fully padded: position 0 (bos) is always a valid key
    assert all(p[0] == 0 for p in pad)


def test_select_by_hand():
    # one utterance, N = 3, Lc = 1; hypotheses [4], [5], [] ; lp rows [j = 0, j = 1]
    hyps = [[[4], [5], []]]
    lp = [[-1.0, -0.5], [-0.25, -1.25], [-3.0, 99.0]]  # att = -1.5, -1.5, -3 (99: past len)
    ctc = [[-2.0, -4.0, -1.0]]
    # ctc_weight 0: att alone; 0 and 1 tie at -1.5 exactly -> the smaller k
    (k, toks, att, tot, resc), = rr.select(lp, hyps, ctc, [1], 3, 0.0)
    assert att == [-1.5, -1.5, -3.0] and tot == [-1.5, -1.5, -3.0]
    assert (k, toks, resc) == (0, [4], True)
    # ctc_weight 1: totals -3.5, -5.5, -4.0
    (k, toks, att, tot, _), = rr.select(lp, hyps, ctc, [1], 3, 1.0)
    assert tot == [-3.5, -5.5, -4.0] and (k, toks) == (0, [4])
    # ctc_weight 0.25: -2.0, -2.5, -3.25; with att of entry 1 better it wins at weight 0.25
    lp2 = [[-1.0, -0.5], [-0.25, -0.25], [-3.0, 0.0]]
    (k, toks, att, tot, _), = rr.select(lp2, hyps, ctc, [1], 3, 0.25)
    assert tot == [-2.0, -1.5, -3.25] and (k, toks) == (1, [5])
    # ok = 0: entry 0 whatever the scores say, not rescored, att 0 / total -inf
    (k, toks, att, tot, resc), = rr.select(lp2, hyps, ctc, [0], 3, 0.25)
    assert (k, toks, resc) == (0, [4], False) and att == [0.0] * 3 and tot == [-INF] * 3
    # an absent slot (two live entries of three) never wins and reads att 0 / total -inf
    (k, toks, att, tot, _), = rr.select(lp2, [[[4], [5]]], ctc, [1], 3, 0.25)
    assert k == 1 and att[2] == 0.0 and tot[2] == -INF


def test_scorer_by_hand():
    # 2 rows x 3 tokens, d = 2. Row 0: h = (1, 0) -> logits (ln 1, ln 2, ln 5) + bias 0, so
    # softmax = (1/8, 2/8, 5/8); row 1: h = (0, 1) -> logits (0, 0, 0) + bias: uniform.
    W = np.array([[math.log(1.0), 0.0], [math.log(2.0), 0.0], [math.log(5.0), 0.0]])
    h = np.array([[1.0, 0.0], [0.0, 1.0]])
    lp, mx = rr.seq_logprob(h, W, None, [2, 0])
    assert abs(lp[0] - math.log(5 / 8)) < 1e-15 and abs(lp[1] - math.log(1 / 3)) < 1e-15
    assert abs(mx - math.log(5.0)) < 1e-15
    # the bias shifts row 1 to (1/8, 2/8, 5/8) too; a skipped row gives 0
    lp, _ = rr.seq_logprob(h, W * 0.0, np.log(np.array([1.0, 2.0, 5.0])), [-1, 1])
    assert lp[0] == 0.0 and abs(lp[1] - math.log(2 / 8)) < 1e-15


@pytest.mark.parametrize("case", [(3, 17, 7, 10), (4, 64, 40, 4), (2, 16, 5004, 10),
                                  (2, 40, 12, 32)])
def test_nbest_oracle_matches_beam_ref(case):
    B, T, V, beam = case
    logits = ctc_like_logits(77, B, T, V)
    lens = ragged_lens(77, B, T)
    for b in range(B):
        x = logits[b, :lens[b]]
        ref = beam_search(x, beam, 3, 20)
        got = rr.nbest_search(x, beam, 3, 20)
        assert got.hyps[0] == ref.tokens and got.scores[0] == ref.score
        assert got.hyps == ref.final_beam
        assert got.margin <= ref.margin
        assert all(a >= b_ for a, b_ in zip(got.scores, got.scores[1:]))
        if lens[b] == 0:
            assert got.hyps == [[]] and got.scores == [0.0]


def test_new_entries_reject_bad_arguments_without_gpu():
    """Every check below fails before any HIP call, so it is safe with no device."""
    from onebit_asr import _lib

    lib = _lib.load()
    f = 0x1000
    big = 1 << 30
    NULL, SHAPE, WS, ALIGN = -1, -2, -4, -5
    # n-best beam search: logits, lens, B, T, V, blank, beam, top_k, nbest, ws, bytes, outs...
    nb = lib.ob_ctc_beam_search_nbest
    assert nb(f, f, 2, 8, 5, 3, 10, 20, 11, f, big, f, f, f, f, None) == SHAPE   # nbest > beam
    assert nb(f, f, 2, 8, 5, 3, 10, 20, 0, f, big, f, f, f, f, None) == SHAPE
    assert nb(f, f, 2, 8, 5, 3, 33, 20, 4, f, big, f, f, f, f, None) == SHAPE    # beam > 32
    assert nb(f, f, 2, 8, 5, 5, 10, 20, 4, f, big, f, f, f, f, None) == SHAPE    # blank >= V
    assert nb(f, f, 2, 8, 5, 3, 10, 20, 4, f, big, f, f, f, None, None) == NULL  # score needed
    assert nb(f, None, 2, 8, 5, 3, 10, 20, 4, f, big, f, f, f, f, None) == NULL
    assert nb(f, f, 2, 8, 5, 3, 10, 20, 4, f, big, f, f, f, 0x1004, None) == ALIGN
    assert nb(f, f, 2, 8, 5, 3, 10, 20, 4, f, big, 0x1002, f, f, f, None) == ALIGN
    need = lib.ob_ctc_beam_search_nbest_workspace(2, 8, 5, 10, 20)
    assert need == lib.ob_ctc_beam_search_workspace(2, 8, 5, 10, 20) > 0
    assert nb(f, f, 2, 8, 5, 3, 10, 20, 4, f, need - 1, f, f, f, f, None) == WS
    assert nb(f, f, 0, 8, 5, 3, 10, 20, 4, None, 0, None, None, None, None, None) == 0  # B == 0
    # grouped attention: q, sq, k, sk, v, sv, kmask, causal, B, group, H, Lq, Lk, dh, ctx
    ga = lib.ob_decattn_fwd_grouped
    assert ga(f, 64, f, 128, f, 128, None, 0, 2, 3, 4, 5, 257, 16, f, None) == SHAPE  # Lk > 256
    assert ga(f, 64, f, 128, f, 128, None, 0, 2, 0, 4, 5, 9, 16, f, None) == SHAPE    # group 0
    assert ga(f, 64, f, 128, f, 128, None, 0, 2, 3, 4, 5, 9, 20, f, None) == SHAPE    # dh
    assert ga(f, 32, f, 128, f, 128, None, 0, 2, 3, 4, 5, 9, 16, f, None) == SHAPE    # sq < H dh
    assert ga(None, 64, f, 128, f, 128, None, 0, 2, 3, 4, 5, 9, 16, f, None) == NULL
    assert ga(f, 64, f, 128, f, 128, None, 0, 2, 3, 4, 5, 9, 16, 0x1004, None) == ALIGN
    # scorer: hidden, R, d, weight, bias, V, target, ws, bytes, lp
    sc = lib.ob_seq_logprob
    assert sc(f, 4, 20, f, f, 5, f, f, big, f, None) == SHAPE     # d % 16 != 0
    assert sc(f, 4, 272, f, f, 5, f, f, big, f, None) == SHAPE    # d > 256
    assert sc(f, 4, 16, f, f, 0, f, f, big, f, None) == SHAPE     # V < 1
    assert sc(f, -1, 16, f, f, 5, f, f, big, f, None) == SHAPE
    assert sc(None, 4, 16, f, f, 5, f, f, big, f, None) == NULL
    assert sc(f, 4, 16, f, f, 5, None, f, big, f, None) == NULL   # target
    assert sc(0x1004, 4, 16, f, f, 5, f, f, big, f, None) == ALIGN  # hidden rows: 16 bytes
    assert sc(f, 4, 16, 0x1008, f, 5, f, f, big, f, None) == ALIGN
    assert sc(f, 4, 16, f, f, 5, f, 0x1004, big, f, None) == ALIGN
    assert lib.ob_seq_logprob_workspace(4, 20, 5) == 0
    need = lib.ob_seq_logprob_workspace(130, 144, 5004)
    # at most a (max, sum) pair per row and 64-column tile + the target's logit: no [R][V]
    assert 0 < need <= 130 * (math.ceil(5004 / 64) * 8 + 4) + 8 < 130 * 5004 * 4 // 6
    assert sc(f, 130, 144, f, f, 5004, f, f, need - 1, f, None) == WS
    assert sc(f, 0, 144, f, f, 5004, f, None, 0, None, None) == 0   # R == 0: no launch
    assert sc(f, 4, 16, f, None, 5, f, None, big, f, None) == NULL  # ws
    # prepare: hyp, hyp_len, n_hyp, B, N, T, Lc, bos, eos, pad, tgt_inp, target, tgt_pad, ok
    pr = lib.ob_rescore_prepare
    assert pr(f, f, f, 2, 33, 8, 4, 1, 2, 0, f, f, f, f, None) == SHAPE   # N > 32
    assert pr(f, f, f, 2, 4, 8, -1, 1, 2, 0, f, f, f, f, None) == SHAPE   # Lc < 0
    assert pr(f, f, None, 2, 4, 8, 4, 1, 2, 0, f, f, f, f, None) == NULL
    assert pr(f, f, f, 2, 4, 8, 4, 1, 2, 0, 0x1004, f, f, f, None) == ALIGN  # int64 tgt_inp
    # select: lp, hyp, hyp_len, n_hyp, ctc, ok, B, N, T, Lc, w, out, out_len, best_k, att, total, resc
    se = lib.ob_rescore_select
    assert se(f, f, f, f, f, f, 2, 0, 8, 4, 0.5, f, f, f, f, f, f, None) == SHAPE
    assert se(None, f, f, f, f, f, 2, 4, 8, 4, 0.5, f, f, f, f, f, f, None) == NULL
    assert se(f, f, f, f, f, f, 2, 4, 8, 4, 0.5, f, f, f, f, f, None, None) == NULL
    assert se(f, f, f, f, 0x1004, f, 2, 4, 8, 4, 0.5, f, f, f, f, f, f, None) == ALIGN
    assert se(f, f, f, f, f, f, 2, 4, 8, 4, 0.5, f, f, f, 0x1004, f, f, None) == ALIGN


def test_decoder_switch_still_rejects_unknown_names():
    from onebit_asr.infer import GraphedInference, encode_and_decode

    with pytest.raises(ValueError, match="decoder must be"):
        encode_and_decode(None, {}, decoder="bogus")
    with pytest.raises(ValueError, match="decoder must be"):
        GraphedInference(None, decoder="bogus")


def test_python_surface_argument_checks_on_cpu():
    import torch

    import onebit_asr
    from onebit_asr.infer import attention_rescore, ctc_beam_search_nbest_device, seq_logprob

    assert onebit_asr.ctc_beam_search_nbest_device is ctc_beam_search_nbest_device
    assert onebit_asr.attention_rescore is attention_rescore
    assert callable(onebit_asr.ctc_attention_rescore_batch)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc_beam_search_nbest_device(torch.zeros(1, 2, 5), torch.tensor([2]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seq_logprob(torch.zeros(2, 16), torch.zeros(5, 16), None, torch.zeros(2, dtype=torch.int32))
