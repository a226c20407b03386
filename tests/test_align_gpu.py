"""GPU: CTC forced alignment (csrc/align.hip, ``onebit_asr.align.ctc_forced_align``) against the
float64 oracle of tests/align_ref.py.

Bars, with e = 1e-9 * max(1, lens) (the project's bar for fp64 CTC scores from fp32 logits).
* ``score`` within e of the oracle, -inf exactly where the oracle says so, and then path / span /
  tok_score are -1 / -1 / 0.
* Independent of the oracle's path: ``path`` collapses to the target and is -1 past ``lens``; the
  spans are exactly the runs of the path's token states; the sum of x[t][path[t]] recomputed on the
  host in float64 equals ``score`` within e; each ``tok_score`` equals its span's sum within e.
* Where the oracle's smallest on-path margin is >= 10e, path and span equal the oracle's exactly;
  every utterance of the cases (the five small ones and one with more states than the block has
  threads) must be decisive.
* Exact ties: the hand-derived paths of tests/golden/align_kat.json. Invalid tokens: -inf and -1
  outputs, the batch's other utterances bitwise unaffected. The same bytes in every slot, inside a
  larger padded T' and S with NaN / garbage past the lengths, and in a second run. Every output
  element is written (the outputs start as poison).
* End to end: ``timestamps=True`` leaves tokens / counts / logits bitwise unchanged; greedy and
  beam output always aligns; the graphed alignment replays bitwise and equals the eager call.

Figures seen on an MI355X (each test prints its own, -s): score error 0 (cases 0, 1, 3, 4),
1.4e-14 (case 2) and 1.1e-13 (the 281- and 257-state case); tok_score error at most 7.1e-15; the
host sum of the device path differs from ``score`` by the same amounts. Oracle margins: 1.71
(case 1), 1.09e-1 / 3.12e-1 / 2.09e-1 (case 2), 3.80e-2 / 1.77e-1 (case 3), 1.45e-2 / 1.95e-2 (the
wide case), inf for the forced paths; the smallest is 4.8e3 x 10e, every utterance decisive and
equal to the oracle's path and spans. Case 4 is infeasible, aligned, empty, infeasible. End to end
(random weights, 182 and 87 frames): greedy returns 156 / 75 tokens, align_score -1206.9 / -572.1;
beam 182 / 87 tokens, -1209.8 / -573.7; attention (max_len 12) aligns both utterances.
"""
import functools
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import align_ref as alr

pytestmark = pytest.mark.gpu

NEG_INF = -math.inf
BLANK = 3
POISON_I, POISON_F = 0x5A5A5A5A, 77.0
KAT = json.loads((Path(__file__).parent / "golden" / "align_kat.json").read_text())

#         B  T'   V     lens               tlen
CASES = [(1, 1, 5, (1,), (1,)),
         (3, 7, 9, (7, 7, 3), (3, 0, 2)),
         (4, 61, 35, (61, 20, 1, 40), (12, 10, 1, 20)),
         (2, 256, 5004, (256, 130), (64, 40)),
         (4, 7, 9, (2, 7, 0, 1), (2, 5, 0, 2))]
# 2 tlen + 1 above the block's 256 threads (281 and 257 states: several states per thread)
WIDE = 5
CASES.append((2, 300, 9, (300, 290), (140, 128)))


@functools.lru_cache(maxsize=None)
def _case(i):
    """(z, targets, x per utterance, the oracle's result per utterance) of case i; read-only."""
    B, Tp, V, lens, tlen = CASES[i]
    rng = np.random.default_rng(9300 + i)
    z = (rng.standard_normal((B, Tp, V)) * 2).astype(np.float32)
    S = max(tlen)
    tg = rng.integers(4, V, size=(B, S)).astype(np.int32)
    for u in range(1, S, 3):
        tg[:, u] = tg[:, u - 1]
    x = [alr.log_softmax64(z[b, :lens[b]]) for b in range(B)]
    ref = [alr.viterbi(x[b], tg[b, :tlen[b]], BLANK) for b in range(B)]
    for a in (z, tg):
        a.setflags(write=False)
    return z, tg, x, ref


def _align(gpu, z, lens, tg, tlen, blank=BLANK):
    """``ob_ctc_align`` on poisoned outputs -> numpy (path, span, tok_score, score)."""
    from onebit_asr import _lib

    lib = _lib.load()
    B, Tp, V = z.shape
    S = tg.shape[1]
    zt = torch.from_numpy(np.ascontiguousarray(z)).to(gpu)
    ln = torch.tensor(lens, dtype=torch.int64, device=gpu)
    tgt = torch.from_numpy(np.ascontiguousarray(tg, dtype=np.int32)).to(gpu)
    tl = torch.tensor(tlen, dtype=torch.int32, device=gpu)
    path = torch.full((B, Tp), POISON_I, dtype=torch.int32, device=gpu)
    span = torch.full((B, S, 2), POISON_I, dtype=torch.int32, device=gpu)
    tok = torch.full((B, S), POISON_F, dtype=torch.float64, device=gpu)
    score = torch.full((B,), POISON_F, dtype=torch.float64, device=gpu)
    need = lib.ob_ctc_align_workspace(B, Tp, S)
    assert need > 0
    ws = torch.empty((need // 8,), dtype=torch.int64, device=gpu)
    _lib.check(lib.ob_ctc_align(zt.data_ptr(), ln.data_ptr(), tgt.data_ptr(), tl.data_ptr(), B, Tp,
                                V, S, blank, ws.data_ptr(), need, path.data_ptr(), span.data_ptr(),
                                tok.data_ptr(), score.data_ptr(), _lib.stream_of(zt)),
               "ob_ctc_align")
    torch.cuda.synchronize()
    out = tuple(t.cpu().numpy() for t in (path, span, tok, score))
    # output completeness: nothing keeps its poison
    assert not (out[0] == POISON_I).any() and not (out[1] == POISON_I).any()
    assert not (out[2] == POISON_F).any() and not (out[3] == POISON_F).any()
    return out


def _runs(path, blank):
    """Maximal runs of equal non-blank ids: [(token, first frame, last frame + 1)]."""
    runs, t = [], 0
    while t < len(path):
        e = t
        while e < len(path) and path[e] == path[t]:
            e += 1
        if path[t] != blank:
            runs.append((int(path[t]), t, e))
        t = e
    return runs


def _check_utterance(x, target, T, got, ref, where):
    """One utterance against the bars of the module docstring -> (score error, tok_score error,
    host-sum error, margin / e)."""
    path, span, tok, score = got
    L = len(target)
    e = 1e-9 * max(1, T)
    assert (path[T:] == -1).all() and (span[L:] == -1).all() and (tok[L:] == 0).all(), where
    if ref.score == NEG_INF:
        assert score == NEG_INF, (where, score)
        assert (path == -1).all() and (span == -1).all() and (tok == 0).all(), where
        return 0.0, 0.0, 0.0, math.inf
    err = abs(score - ref.score)
    assert err <= e, (where, score, ref.score)
    p = path[:T].tolist()
    assert alr.collapse(p, BLANK) == list(target), where
    runs = _runs(p, BLANK)
    assert [r[0] for r in runs] == list(target), where
    assert span[:L].tolist() == [[f, en] for _, f, en in runs], where
    host = 0.0
    for t, c in enumerate(p):
        host += float(x[t][c])
    assert abs(host - score) <= e, (where, host, score)
    tok_err = 0.0
    for u, (c, f, en) in enumerate(runs):
        want = 0.0
        for t in range(f, en):
            want += float(x[t][c])
        tok_err = max(tok_err, abs(tok[u] - want))
    assert tok_err <= e, (where, tok_err)
    assert ref.margin >= 10 * e, (where, "not decisive", ref.margin)
    assert p == ref.path and span[:L].tolist() == [list(s) for s in ref.spans], where
    return err, tok_err, abs(host - score), ref.margin / e


@pytest.mark.parametrize("i", range(len(CASES)))
def test_alignment_matches_float64_oracle(gpu, i):
    B, Tp, V, lens, tlen = CASES[i]
    z, tg, x, ref = _case(i)
    got = _align(gpu, z, lens, tg, tlen)
    worst = [0.0, 0.0, 0.0]
    margins = []
    for b in range(B):
        r = _check_utterance(x[b], tg[b, :tlen[b]], lens[b], [g[b] for g in got], ref[b], (i, b))
        worst = [max(w, v) for w, v in zip(worst, r[:3])]
        margins.append(ref[b].margin)
    feasible = [r.score != NEG_INF for r in ref]
    print(f"case {i}: B={B} T'={Tp} V={V}: score err {worst[0]:.2e}, tok_score err {worst[1]:.2e}, "
          f"host sum err {worst[2]:.2e}, margins {['%.2e' % m for m in margins]}, feasible "
          f"{feasible}")
    if i == WIDE:
        assert all(feasible) and min(2 * n + 1 for n in tlen) > 256
    if i == 4:   # two infeasible utterances, a repeat that fits exactly, an empty one
        assert feasible == [False, True, True, False]
        assert got[3][2] == 0.0 and (got[0][2] == -1).all()
    if i == 1:   # a blank-only utterance; a ∅ a in 3 frames
        assert (got[0][1] == BLANK).all()
        assert got[0][2, :3].tolist() == [tg[2, 0], BLANK, tg[2, 0]]


def test_exact_ties_follow_the_rules(gpu):
    cases = KAT["cases"]
    B, Tp, S = len(cases), max(c["T"] for c in cases), max(len(c["target"]) for c in cases)
    z = np.zeros((B, Tp, KAT["V"]), np.float32)
    tg = np.zeros((B, S), np.int32)
    for b, c in enumerate(cases):
        tg[b, :len(c["target"])] = c["target"]
    lens = [c["T"] for c in cases]
    path, span, tok, score = _align(gpu, z, lens, tg, [len(c["target"]) for c in cases],
                                    KAT["blank"])
    for b, c in enumerate(cases):
        T, L = c["T"], len(c["target"])
        assert path[b].tolist() == c["path"] + [-1] * (Tp - T), c
        assert span[b].tolist() == c["spans"] + [[-1, -1]] * (S - L), c
        if c["feasible"]:
            assert abs(score[b] - T * math.log(0.25)) <= 1e-9 * T, c
            for u, (f, e) in enumerate(c["spans"]):
                assert abs(tok[b, u] - (e - f) * math.log(0.25)) <= 1e-9 * T, c
        else:
            assert score[b] == NEG_INF and (tok[b] == 0).all(), c


def test_invalid_tokens_are_infeasible_and_never_indexed(gpu):
    B, Tp, V, lens, tlen = CASES[2]
    z, tg, _, _ = _case(2)
    clean = _align(gpu, z, lens, tg, tlen)
    assert clean[3][1] != NEG_INF
    for bad in (V, -1, BLANK, 2 ** 31 - 1, -2 ** 31):
        t2 = tg.copy()
        t2[1, 3] = bad
        got = _align(gpu, z, lens, t2, tlen)
        assert got[3][1] == NEG_INF, bad
        assert (got[0][1] == -1).all() and (got[1][1] == -1).all() and (got[2][1] == 0).all(), bad
        for b in (0, 2, 3):
            for g, c in zip(got, clean):
                assert g[b].tobytes() == c[b].tobytes(), (bad, b)
    # the same value past tlen is padding
    t2 = tg.copy()
    t2[1, tlen[1]:] = V
    for g, c in zip(_align(gpu, z, lens, t2, tlen), clean):
        assert g.tobytes() == c.tobytes()


def test_slot_and_padding_invariance(gpu):
    B, Tp, V, lens, tlen = CASES[2]
    z, tg, _, ref = _case(2)
    S = tg.shape[1]
    base = _align(gpu, z, lens, tg, tlen)
    perm = [2, 0, 3, 1]
    permuted = _align(gpu, z[perm], [lens[p] for p in perm], tg[perm], [tlen[p] for p in perm])
    Tp2, S2 = Tp + 9, S + 7
    z2 = np.full((B, Tp2, V), np.nan, np.float32)
    tg2 = np.full((B, S2), 10 ** 9, np.int32)
    tg2[:, ::2] = -7
    for b in range(B):
        z2[b, :lens[b]] = z[b, :lens[b]]
        tg2[b, :tlen[b]] = tg[b, :tlen[b]]
    padded = _align(gpu, z2, lens, tg2, tlen)
    again = _align(gpu, z2, lens, tg2, tlen)
    for g, a in zip(padded, again):
        assert g.tobytes() == a.tobytes()

    def own(out, b, T, L):
        return (out[0][b, :T].tobytes(), out[1][b, :L].tobytes(), out[2][b, :L].tobytes(),
                out[3][b].tobytes())
    for b in range(B):
        want = own(base, b, lens[b], tlen[b])
        assert own(permuted, perm.index(b), lens[b], tlen[b]) == want, b
        assert own(padded, b, lens[b], tlen[b]) == want, b
        assert own(again, b, lens[b], tlen[b]) == want, b
        assert (padded[0][b, lens[b]:] == -1).all() and (padded[1][b, tlen[b]:] == -1).all()
        assert (padded[2][b, tlen[b]:] == 0).all()
        assert ref[b].score != NEG_INF and base[3][b] != NEG_INF


def test_python_entry_equals_the_c_entry(gpu):
    from onebit_asr.align import ctc_forced_align, token_confidence

    B, Tp, V, lens, tlen = CASES[2]
    z, tg, _, _ = _case(2)
    S = tg.shape[1]
    raw = _align(gpu, z, lens, tg, tlen)
    zt = torch.from_numpy(np.ascontiguousarray(z)).to(gpu)
    # int64 targets, wider than S and narrowed by max_target_len, lens / target_lens on the host
    wide = torch.full((B, S + 5), 10 ** 12, dtype=torch.int64)
    wide[:, :S] = torch.from_numpy(np.ascontiguousarray(tg)).long()
    al = ctc_forced_align(zt, torch.tensor(lens), wide, torch.tensor(tlen), BLANK,
                          max_target_len=S)
    assert al.span.shape == (B, S, 2) and al.tok_score.dtype == al.score.dtype == torch.float64
    for g, r in zip(al, raw):
        assert g.cpu().numpy().tobytes() == r.tobytes()
    conf = token_confidence(al.span, al.tok_score).cpu().numpy()
    assert conf.dtype == np.float32 and conf.shape == (B, S)
    frames = (raw[1][..., 1] - raw[1][..., 0]).clip(min=1)
    want = np.where(raw[1][..., 0] >= 0, np.exp(raw[2] / frames), 0.0)
    assert np.abs(conf - want).max() <= 1e-6 and (conf[raw[1][..., 0] < 0] == 0).all()
    assert ((conf >= 0) & (conf <= 1)).all()
    # S == 0 and an unsupported shape
    al0 = ctc_forced_align(zt, torch.tensor(lens), wide, torch.zeros(B, dtype=torch.int64), BLANK,
                           max_target_len=0)
    assert al0.span.shape == (B, 0, 2)
    p0 = al0.path.cpu().numpy()
    for b in range(B):
        assert (p0[b, :lens[b]] == BLANK).all() and (p0[b, lens[b]:] == -1).all()
    with pytest.raises(ValueError, match="not supported"):
        ctc_forced_align(zt, torch.tensor(lens), torch.zeros(B, 512, dtype=torch.int64),
                         torch.tensor(tlen))


# ------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_and_batch():
    from onebit_asr.conformer import ConformerASR
    from onebit_asr.data import CFG1, synthetic_batch

    torch.manual_seed(0)
    model = ConformerASR(80, 5004, **CFG1).to("cuda:0").eval()
    return model, synthetic_batch([734, 349], [27, 12], device="cuda:0")


def _collapsed(row, T):
    return alr.collapse(row[:T].tolist(), BLANK)


@pytest.mark.parametrize("decoder", ["greedy", "beam"])
def test_timestamps_for_the_ctc_decoders(gpu, decoder):
    from onebit_asr.infer import encode_and_decode

    model, batch = _model_and_batch()
    out0, cnt0, logits0 = encode_and_decode(model, batch, decoder=decoder, beam_size=4)
    info = {}
    out, cnt, logits = encode_and_decode(model, batch, decoder=decoder, beam_size=4, info=info,
                                         timestamps=True)
    assert torch.equal(out, out0) and torch.equal(cnt, cnt0) and torch.equal(logits, logits0)
    B, Tp, _ = logits.shape
    assert info["frame_path"].shape == (B, Tp) and info["align_score"].shape == (B,)
    assert info["span"].shape[0] == B and info["span"].shape[2] == 2
    assert info["tok_score"].shape == info["span"].shape[:2]
    fp = info["frame_path"].cpu().numpy()
    span = info["span"].cpu().numpy()
    lens = (fp != -1).sum(1)
    score = info["align_score"].cpu().numpy()
    assert np.isfinite(score).all()
    for b in range(B):
        n = int(cnt[b])
        assert _collapsed(fp[b], lens[b]) == out[b, :n].tolist()
        assert (span[b, :n, 0] >= 0).all() and (span[b, :n, 1] > span[b, :n, 0]).all()
        assert (span[b, n:] == -1).all()
        if decoder == "greedy":
            am = logits[b].argmax(-1).cpu().numpy()
            assert _collapsed(am, lens[b]) == _collapsed(fp[b], lens[b])
    print(f"{decoder}: frames {lens.tolist()}, tokens {cnt.tolist()}, align_score {score}")


def test_timestamps_for_the_attention_decoder(gpu):
    from onebit_asr.infer import encode_and_decode

    model, batch = _model_and_batch()
    info = {}
    out, cnt, logits = encode_and_decode(model, batch, decoder="attention", beam_size=4, max_len=12,
                                         info=info, timestamps=True)
    out0, cnt0, logits0 = encode_and_decode(model, batch, decoder="attention", beam_size=4,
                                            max_len=12)
    assert torch.equal(out, out0) and torch.equal(cnt, cnt0) and torch.equal(logits, logits0)
    score = info["align_score"].cpu().numpy()
    span, fp = info["span"].cpu().numpy(), info["frame_path"].cpu().numpy()
    assert span.shape == (2, 12, 2) and "hyp" in info
    for b in range(2):
        n = int(cnt[b])
        if score[b] == NEG_INF:
            assert (span[b] == -1).all() and (fp[b] == -1).all()
        else:
            assert np.isfinite(score[b]) and (span[b, :n, 0] >= 0).all()
            assert alr.collapse(fp[b][fp[b] != -1].tolist(), BLANK) == out[b, :n].tolist()
    print(f"attention: tokens {cnt.tolist()}, align_score {score}")


def test_graphed_timestamps_replay_bitwise_and_equal_eager(gpu):
    from onebit_asr.align import ctc_forced_align
    from onebit_asr.infer import GraphedInference

    model, batch = _model_and_batch()
    gi = GraphedInference(model, act_quant=None, timestamps=True)
    keys = ("span", "tok_score", "align_score", "frame_path")
    runs = []
    for _ in range(3):
        out, cnt, logits = gi.run(batch)
        runs.append([gi.info[k].clone() for k in keys] + [out.clone(), cnt.clone(), logits.clone()])
    assert gi.graph is not None
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert torch.equal(a, b)
    _, mask, _ = model(batch, precision=2)
    out, cnt, logits = runs[0][4:]
    al = ctc_forced_align(logits, mask.sum(dim=1), out, cnt)
    for got, want in zip(runs[0][:4], (al.span, al.tok_score, al.score, al.path)):
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert torch.isfinite(al.score).all()
