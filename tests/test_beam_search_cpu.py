"""CPU: the beam-search test oracle (tests/ctc_beam_ref.py) against hand-derived known answers
and against recorded output of the reference decoder (metrics.py:74-145); argument validation
of ob_ctc_beam_search before any HIP call; the host-side WER helpers of onebit_asr.metrics."""
import json
import math

import numpy as np
import pytest

from ctc_beam_ref import (beam_search, beam_search_batch, beam_search_fresh_ids, ctc_like_logits,
                          ragged_lens)


def _load(golden_dir, name):
    return json.loads((golden_dir / name).read_text())


def test_oracle_matches_hand_derived_answers(golden_dir):
    kat = _load(golden_dir, "beam_kat.json")
    assert "derived by hand" in kat["_about"]
    names = [c["name"] for c in kat["cases"]]
    assert {"a _ a", "a a b b", "L = 0"} <= set(names)
    from oracle.decode_oracle import np_ctc_greedy_decode

    for c in kat["cases"]:
        x = np.asarray(c["logits"], np.float32)[:c["len"]]
        got = beam_search(x, kat["beam_size"], kat["blank_id"], kat["top_k_per_t"])
        assert got.tokens == c["tokens"], c["name"]
        if c["score"] is not None:
            assert abs(got.score - c["score"]) <= 1e-12, (c["name"], got.score)
        if c["len"]:
            assert np_ctc_greedy_decode(x, kat["blank_id"]) == c["greedy"], c["name"]
    a_a = kat["cases"][names.index("a _ a")]
    assert a_a["tokens"] == [4] and a_a["greedy"] == [4, 4]  # the reference's repeat rule
    assert abs(a_a["score"] - (-0.2268914)) < 1e-7  # ln(p^3 + 2 p^2 q + q^3), see _about


def test_oracle_matches_recorded_reference_output(golden_dir):
    ref = _load(golden_dir, "beam_ref.json")
    assert len(ref["cases"]) >= 8
    for c in ref["cases"]:
        x = np.asarray(c["logits"], np.float32)
        assert x.shape == (c["T"], c["V"]) and c["top_k_per_t"] < c["V"]  # top-k applies
        # the fixture is the generator's logits, bit for bit
        assert np.array_equal(x, ctc_like_logits(c["seed"], 1, c["T"], c["V"])[0])
        got = beam_search(x, c["beam_size"], c["blank_id"], c["top_k_per_t"])
        assert got.margin >= 1e-4, (c["seed"], got.margin)
        assert got.tokens == c["tokens"], c["seed"]


def test_beam_search_argument_validation_without_gpu():
    """Every check below fails (or returns) before any HIP call, so it is safe with no device."""
    from onebit_asr import _lib

    lib = _lib.load()
    fake = 0x1000  # never dereferenced
    need = lib.ob_ctc_beam_search_workspace(2, 16, 40, 10, 20)
    assert need > 2 * 16 * 21 * 8  # at least the [B][T][K+1] fp64 candidates

    def call(logits=fake, lens=fake, B=2, T=16, V=40, blank=3, beam=10, top_k=20, ws=fake,
             ws_bytes=need, out=fake, out_len=fake, score=fake):
        return lib.ob_ctc_beam_search(logits, lens, B, T, V, blank, beam, top_k, ws, ws_bytes,
                                      out, out_len, score, None)

    for bad in (dict(B=-1), dict(T=-1), dict(V=0), dict(blank=-1), dict(blank=40), dict(beam=0),
                dict(beam=33), dict(top_k=0), dict(top_k=65)):
        assert call(**bad) == -2, bad  # OB_ERR_SHAPE
    for bad in (dict(logits=None), dict(lens=None), dict(ws=None), dict(out=None),
                dict(out_len=None)):
        assert call(**bad) == -1, bad  # OB_ERR_NULL
    for bad in (dict(logits=0x1002), dict(out=0x1002), dict(out_len=0x1001), dict(ws=0x1004),
                dict(score=0x1004), dict(lens=0x1004)):
        assert call(**bad) == -5, bad  # OB_ERR_ALIGN
    assert call(ws_bytes=need - 1) == -4  # OB_ERR_WORKSPACE
    assert call(B=0) == 0  # nothing to do: OB_OK without a launch
    assert call(B=0, logits=None, lens=None, ws=None, ws_bytes=0, out=None, out_len=None,
                score=None) == 0
    assert call(B=0, beam=0) == -2  # the argument limits hold for an empty batch too

    def stage(k, **kw):  # the two launches on their own: ob_ctc_beam_search_stage
        a = dict(logits=fake, lens=fake, out=fake, out_len=fake, score=fake, ws=fake, ws_bytes=need)
        a.update(kw)
        return lib.ob_ctc_beam_search_stage(a["logits"], a["lens"], 2, 16, 40, 3, 10, 20, k,
                                            a["ws"], a["ws_bytes"], a["out"], a["out_len"],
                                            a["score"], None)

    assert stage(-1) == -2 and stage(3) == -2
    assert stage(1, logits=None) == -1 and stage(2, out=None) == -1 and stage(2, out_len=None) == -1
    assert stage(1, ws_bytes=need - 1) == -4 and stage(2, ws_bytes=need - 1) == -4
    assert stage(2, ws=0x1004) == -5

    ws = lib.ob_ctc_beam_search_workspace
    base = dict(B=2, T=16, V=40, beam=10, top_k=20)
    order = ("B", "T", "V", "beam", "top_k")
    grow = dict(B=[1, 2, 3, 8, 256], T=[1, 2, 16, 17, 249], V=[1, 5, 19, 20, 21, 64, 5004],
                beam=[1, 2, 10, 16, 32], top_k=[1, 2, 20, 39, 40, 64])
    for name, values in grow.items():
        sizes = [ws(*[dict(base, **{name: v})[k] for k in order]) for v in values]
        assert all(s > 0 and s % 8 == 0 for s in sizes), (name, sizes)
        assert sizes == sorted(sizes), (name, sizes)  # never shrinks as the argument grows
        assert sizes[-1] > sizes[0], (name, sizes)
    # V stops mattering once it exceeds top_k (the workspace never holds V-sized rows)
    assert ws(2, 16, 21, 10, 20) == ws(2, 16, 5004, 10, 20)
    assert ws(0, 16, 40, 10, 20) == 0 and ws(2, 0, 40, 10, 20) > 0  # the prefix table's minimum
    for bad in ((-1, 16, 40, 10, 20), (2, -1, 40, 10, 20), (2, 16, 0, 10, 20), (2, 16, 40, 0, 20),
                (2, 16, 40, 33, 20), (2, 16, 40, 10, 0), (2, 16, 40, 10, 65)):
        assert ws(*bad) == 0, bad


class _StubProcessor:
    """Stands in for a SentencePiece processor: decode(piece ids) -> text."""

    def __init__(self):
        self.calls = []

    def decode(self, pieces):
        self.calls.append(list(pieces))
        return " ".join(f"w{p}" for p in pieces)


def test_wer_helpers():
    import torch

    from onebit_asr import metrics
    from onebit_asr.metrics import compute_wer, ids_to_text, levenshtein_distance

    assert levenshtein_distance([], []) == 0
    assert levenshtein_distance(["a", "b"], []) == 2
    assert levenshtein_distance([], ["a"]) == 1
    assert levenshtein_distance("kitten", "sitting") == 3
    assert levenshtein_distance(["a", "b", "c"], ["a", "c"]) == 1  # one deletion
    assert levenshtein_distance(["a", "c"], ["a", "b", "c"]) == 1  # one insertion
    assert levenshtein_distance(["a", "b", "c"], ["a", "x", "c"]) == 1  # one substitution
    assert levenshtein_distance(["a", "b"], ["b", "a"]) == 2
    assert compute_wer(["the cat sat", "hello"], ["the cat sat", "hello"]) == (0, 4)
    assert compute_wer(["the cat sat", "hello world"], ["the bat sat down", ""]) == (4, 5)
    assert compute_wer([], []) == (0, 0)

    sp = _StubProcessor()
    assert ids_to_text([4, 0, 3, 9, 1, 2, 5], sp) == "w0 w5 w1"  # pad/bos/eos/blank dropped
    assert sp.calls == [[0, 5, 1]]
    assert ids_to_text(torch.tensor([6, 3, 4]), sp) == "w2 w0"
    assert ids_to_text([0, 1, 2, 3], sp) == "" and len(sp.calls) == 2  # nothing to decode
    assert ids_to_text([10, 12], sp, token_offset=10) == "w0 w2"
    # the reference module's decoder names are here too (eval.py:17-21 imports them)
    for name in ("ctc_beam_search", "ctc_beam_search_batch", "ctc_greedy_decode"):
        assert callable(getattr(metrics, name))
    import onebit_asr

    assert onebit_asr.ctc_beam_search_batch is metrics.ctc_beam_search_batch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.ctc_beam_search(torch.zeros(3, 6))


def test_oracle_margin_and_reentry_bookkeeping():
    """The oracle's side outputs, on cases small enough to reason about."""
    x = np.full((1, 6), -1.0, np.float32)
    x[0, 4] = 3.0
    r = beam_search(x, beam=10, blank=3, top_k=None)
    lp = x[0].astype(np.float64) - math.log(np.exp(x[0].astype(np.float64)).sum())
    assert r.tokens == [4] and abs(r.score - lp[4]) < 1e-15
    assert abs(r.margin - (lp[4] - lp[0])) < 1e-12  # best vs second of the final beam
    assert len(r.final_beam) == 6 and r.reentries == 0 and r.merges == 0
    # top-k boundary: bit-equal logits at ranks K and K + 1 give margin 0
    y = np.array([[5, 4, 3, 2, 1, 1, 0]], np.float32)
    assert beam_search(y, beam=3, blank=3, top_k=5).margin == 0.0
    assert beam_search(np.zeros((0, 6), np.float32)).tokens == []


def test_gpu_inputs_exercise_merging_and_prefix_identity():
    """What tests/test_beam_search_gpu.py relies on, from the oracle alone: its shape cases do
    merge extensions into live prefixes, and its prefix-identity input separates a search with
    canonical prefix ids from one that gives a rebuilt prefix a fresh id."""
    merges = 0
    for seed, (B, T, V, beam, top_k) in ((1001, (3, 17, 7, 10, 20)), (1002, (4, 64, 40, 10, 20)),
                                         (1006, (3, 48, 70, 16, 32)), (1007, (2, 40, 12, 32, 20))):
        x = ctc_like_logits(seed, B, T, V)
        merges += sum(r.merges for r in beam_search_batch(x, ragged_lens(seed, B, T), beam, 3, top_k))
    assert merges >= 100
    x = ctc_like_logits(3050, 4, 48, 12)
    for b in range(4):
        good = beam_search(x[b], 4, 3, 20)
        wrong = beam_search_fresh_ids(x[b], 4, 3, 20)
        if b == 1:
            assert wrong.merges == 1 and wrong.tokens != good.tokens
            assert abs(wrong.score - good.score) > 0.1
        else:  # no missed merge: the variant is the same search, bit for bit
            assert wrong.merges == 0 and wrong.tokens == good.tokens and wrong.score == good.score
