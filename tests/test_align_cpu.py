"""CPU: the oracle of CTC forced alignment (tests/align_ref.py) against a brute-force enumeration
of every alignment and against paths derived by hand (tests/golden/align_kat.json); the argument
checks of the new C entry points, which fail before any HIP call; the Python surface.

Figures seen (-s): Viterbi against enumeration, worst difference 0 over the four shapes (every
target of up to 3 tokens; both add the path's terms in frame order), -inf exactly where no alignment
exists: 12, 10, 3 and 0 targets.
"""
import inspect
import itertools
import json
import math
from pathlib import Path

import numpy as np
import pytest

import align_ref as alr

NEG_INF = -math.inf
KAT = json.loads((Path(__file__).parent / "golden" / "align_kat.json").read_text())


@pytest.mark.parametrize("T,V", [(1, 3), (2, 3), (4, 4), (5, 3)])
def test_viterbi_matches_enumeration(T, V):
    blank = V - 1
    rng = np.random.default_rng(100 * T + V)
    x = alr.log_softmax64(rng.standard_normal((T, V)).astype(np.float32) * 2.0)
    best = alr.brute_force(x, blank)
    worst, n_inf = 0.0, 0
    for n in range(4):
        for g in itertools.product(range(V - 1), repeat=n):
            r = alr.viterbi(x, g, blank)
            want = best.get(g, NEG_INF)
            if want == NEG_INF:
                n_inf += 1
                assert r.score == NEG_INF and r.path == [-1] * T, (g, r)
                assert r.spans == [(-1, -1)] * n and r.tok_scores == [0.0] * n
                continue
            worst = max(worst, abs(r.score - want))
            # the returned path is an alignment of g with the returned score, spans and sums
            assert alr.collapse(r.path, blank) == list(g)
            assert abs(sum(x[t][c] for t, c in enumerate(r.path)) - r.score) <= 1e-12
            for u, (f, e) in enumerate(r.spans):
                assert all(r.path[t] == g[u] for t in range(f, e)) and f < e
                assert abs(sum(x[t][g[u]] for t in range(f, e)) - r.tok_scores[u]) <= 1e-12
            assert r.margin >= 0
    print(f"T={T} V={V}: worst {worst:.2e}, {n_inf} without an alignment")
    assert worst <= 1e-12
    if (T, V) == (4, 4):
        assert alr.viterbi(x, [0, 0, 0], blank).score == NEG_INF     # needs 5 frames
        assert alr.viterbi(x, [0, 0], blank).score != NEG_INF


def test_oracle_rejects_invalid_tokens():
    x = alr.log_softmax64(np.zeros((4, 5), np.float32))
    for bad in (5, -1, 3):
        assert alr.viterbi(x, [0, bad], 3).score == NEG_INF
    assert alr.viterbi(x[:0], [], 3).score == 0.0 and alr.viterbi(x[:0], [0], 3).score == NEG_INF


def test_known_answers_by_hand():
    assert KAT["V"] == 4 and KAT["blank"] == 3
    for c in KAT["cases"]:
        x = np.full((c["T"], 4), math.log(0.25))
        r = alr.viterbi(x, c["target"], 3)
        assert r.path == c["path"], c
        assert [list(s) for s in r.spans] == c["spans"], c
        if c["feasible"]:
            assert abs(r.score - c["T"] * math.log(0.25)) <= 1e-13, c
            assert r.margin == 0.0 or r.margin == math.inf      # only ties, or a forced path
            for (f, e), ts in zip(r.spans, r.tok_scores):
                assert abs(ts - (e - f) * math.log(0.25)) <= 1e-13
        else:
            assert r.score == NEG_INF and r.tok_scores == [0.0] * len(c["target"])


def test_argument_validation_without_a_device():
    from onebit_asr import _lib

    lib = _lib.load()
    f = 0x1000
    NULL, SHAPE, WS, ALIGN = -1, -2, -4, -5
    sup = lib.ob_ctc_align_supported
    assert sup(1, 0) and sup(249, 249) and sup(4096, 511)
    assert not sup(4097, 10) and not sup(0, 10) and not sup(100, 512) and not sup(100, -1)
    ws = lib.ob_ctc_align_workspace
    need = ws(2, 7, 5)
    assert need >= 2 * 7 * (6 * 8 + 11) and need % 8 == 0
    assert ws(2, 4096, 511) > 0 and ws(2, 4097, 5) == 0 and ws(2, 7, 512) == 0 and ws(2, 0, 5) == 0
    assert ws(-1, 7, 5) == 0
    big = ws(256, 249, 249)
    print(f"workspace at B=256 T'=249: S=64 {ws(256, 249, 64)} bytes, S=249 {big} bytes")
    assert big == 256 * 249 * (250 * 8 + 499) + 8

    # logits, lens, targets, tlen, B, T', V, S, blank, ws, ws_bytes, path, span, tok_score, score
    def call(**kw):
        args = dict(logits=f, lens=f, targets=f, tlen=f, B=2, Tp=7, V=9, S=5, blank=3, ws=f,
                    ws_bytes=need - 1, path=f, span=f, tok_score=f, score=f)
        args.update(kw)
        return lib.ob_ctc_align(*args.values(), None)
    assert call() == WS                                   # one byte short, everything else valid
    assert call(Tp=4097) == SHAPE and call(Tp=0) == SHAPE and call(S=512) == SHAPE
    assert call(S=-1) == SHAPE and call(V=0) == SHAPE and call(B=-1) == SHAPE
    assert call(blank=9) == SHAPE and call(blank=-1) == SHAPE
    ptrs = ("logits", "lens", "targets", "tlen", "ws", "path", "span", "tok_score", "score")
    for name in ptrs:
        assert call(**{name: None}) == NULL, name
    for name in ("lens", "ws", "tok_score", "score"):                             # 8-byte
        assert call(**{name: 0x3004}) == ALIGN, name
    for name in ("logits", "targets", "tlen", "path", "span"):
        assert call(**{name: 0x3002}) == ALIGN, name
    # S == 0: targets, span and tok_score may be null; the rest may not
    short0 = ws(2, 7, 0) - 1
    assert call(S=0, targets=None, span=None, tok_score=None, ws_bytes=short0) == WS
    assert call(S=0, targets=None, span=None, tok_score=None, score=None) == NULL
    assert call(B=0, **{name: None for name in ptrs}) == 0                        # B == 0

    # the phases on their own: stage 1 needs no outputs, 2 no logits, 3 (no walk) only score
    def stage(k, **kw):
        args = dict(logits=f, lens=f, targets=f, tlen=f, B=2, Tp=7, V=9, S=5, blank=3, stage=k,
                    ws=f, ws_bytes=need - 1, path=f, span=f, tok_score=f, score=f)
        args.update(kw)
        return lib.ob_ctc_align_stage(*args.values(), None)
    assert stage(4) == SHAPE and stage(-1) == SHAPE and stage(0) == WS
    assert stage(1, path=None, span=None, tok_score=None, score=None) == WS
    assert stage(1, logits=None) == NULL
    assert stage(2, logits=None) == WS and stage(2, path=None) == NULL
    assert stage(3, logits=None, path=None, span=None, tok_score=None) == WS
    assert stage(3, score=None) == NULL and stage(0, logits=None) == NULL


def test_python_surface_on_cpu():
    import torch

    import onebit_asr
    from onebit_asr.align import Alignment, ctc_forced_align, span_seconds, token_confidence
    from onebit_asr.infer import GraphedInference, encode_and_decode

    assert onebit_asr.ctc_forced_align is ctc_forced_align
    assert onebit_asr.token_confidence is token_confidence
    assert onebit_asr.span_seconds is span_seconds
    assert Alignment._fields == ("path", "span", "tok_score", "score")
    with pytest.raises(RuntimeError, match="ctc_forced_align runs on the HIP library"):
        ctc_forced_align(torch.zeros(2, 9, 40), torch.tensor([9, 3]),
                         torch.zeros(2, 4, dtype=torch.int64), torch.tensor([4, 2]))

    span = torch.tensor([[[0, 2], [2, 3], [-1, -1]]], dtype=torch.int32)
    start, end = span_seconds(span)
    assert start.tolist() == [[0.0, 0.08, -1.0]] and end.tolist() == [[0.08, 0.12, -1.0]]
    assert span_seconds(span, 0.01)[1].tolist() == [[0.02, 0.03, -1.0]]
    assert "receptive field" in " ".join(span_seconds.__doc__.split())

    ts = torch.tensor([[2 * math.log(0.5), math.log(0.25), 0.0]], dtype=torch.float64)
    conf = token_confidence(span, ts)
    assert conf.dtype == torch.float32
    assert conf.tolist() == [[0.5, 0.25, 0.0]]

    for fn in (encode_and_decode, GraphedInference.__init__):
        p = inspect.signature(fn).parameters
        assert p["timestamps"].default is False
    with pytest.raises(TypeError, match="timestamps"):
        encode_and_decode(None, {}, timestamps=0.3)
    with pytest.raises(TypeError, match="timestamps"):
        GraphedInference(torch.nn.Identity(), act_quant=None, timestamps=1)
    assert GraphedInference(torch.nn.Identity(), act_quant=None, timestamps=True).timestamps


def test_word_spans_groups_pieces_at_the_word_mark():
    import torch

    import onebit_asr
    from onebit_asr.metrics import word_spans

    assert onebit_asr.word_spans is word_spans

    class FakeSpm:
        pieces = ["▁he", "llo", "▁wor", "ld"]

        def id_to_piece(self, i):
            return self.pieces[i]

    ids = [4, 5, 6, 7]
    span = [[0, 2], [2, 3], [5, 6], [6, 9]]
    assert word_spans(ids, span, FakeSpm()) == [("hello", 0, 3), ("world", 5, 9)]
    # tensors; ids below the offset (eos = 2) and tokens without a span are skipped
    ids_t = torch.tensor([4, 2, 5, 6, 7, 4])
    span_t = torch.tensor([[0, 2], [2, 3], [3, 4], [5, 6], [-1, -1], [7, 8]])
    assert word_spans(ids_t, span_t, FakeSpm()) == [("hello", 0, 4), ("wor", 5, 6), ("he", 7, 8)]
    # a transcript that starts inside a word still opens one
    assert word_spans([5, 6], [[1, 2], [2, 4]], FakeSpm()) == [("llo", 1, 2), ("wor", 2, 4)]
    assert word_spans([], [], FakeSpm()) == []
    # another offset
    assert word_spans([0, 1], [[0, 1], [1, 2]], FakeSpm(), token_offset=0) == [("hello", 0, 2)]
