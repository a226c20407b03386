"""GPU: the attention-decoder beam search with a KV cache (csrc/attdec.hip,
onebit_asr/attdec.py, ``decoder="attention"``) against the float64 oracle of tests/attdec_ref.py.

Bars.
* Step attention: 4x the error the existing ``ob_decattn_fwd`` shows against the same float64
  reference on the same data. The last query row of a causal attention sees every key, so the
  comparator runs that row alone (Lq = 1) over the t + 1 keys. Bitwise equal under a permuted
  slot assignment, the unused slots poisoned with NaN.
* ``ob_seq_topk``: lse and values within max(1e-5 * max|logit|, 4 * e_torch), e_torch the error of
  torch's fp32 CPU expression against the same float64 reference (per case, printed); indices
  exact, every reported rank having a float64 gap to the next candidate of >= 10x the measured
  value error (asserted) or being an exact tie of two identical weight rows.
* Beam-step / finalize kernels: equal to the oracle bookkeeping exactly (binary-fraction tables).
* End to end: the step-wise rule of ``attdec_ref.check_search`` with e = 4x the error of the
  existing path (``model.decode_logits`` on the GPU, log-softmax in float64 on the host) on the
  same prefixes; the n-best equals the oracle's exactly where the oracle's smallest margin is
  >= 10e (the four greedy V = 40 cases must be: float64 margins 2.4e-3, 3.8e-3, 8.8e-3, 2.8e-3);
  every returned score within e of its teacher-forced score from ``decoder.hidden`` +
  ``seq_logprob``.
* Graphed: bitwise equal to eager, replays bitwise equal.

Figures seen on an MI355X (each test prints its own, -s): step attention error equal to the
existing forward's on every shape (at most 3.2e-7); ``ob_seq_topk`` error 2.4e-5 at R=130 d=256
V=64 (e_torch 1.9e-5, bar 6.3e-4) and 2.1e-5 at R=130 d=144 V=5004 (bar 6.2e-4); end-to-end
device score error at most 2.1e-6 where e is 1.0e-6 to 7.7e-6, every utterance of every case
decisive (smallest oracle margin 1.3e-4) and equal to the oracle's n-best.
"""
import copy
import functools
import math
import zlib

import numpy as np
import pytest
import torch

import attdec_ref as ar
import rescore_ref as rr

pytestmark = pytest.mark.gpu

NEG_INF = -math.inf


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------
# 1. cached single-query self-attention
# ------------------------------------------------------------------------------------------
#               R  H  dh  L    t
STEP_CASES = [(1, 1, 16, 4, 0), (6, 4, 16, 12, 11), (5, 4, 36, 9, 4), (3, 2, 64, 255, 254),
              (4, 4, 32, 7, 3)]


@functools.lru_cache(maxsize=None)
def _step_case(i):
    R, H, dh, L, t = STEP_CASES[i]
    e = H * dh
    rng = np.random.default_rng(7000 + i)
    qkv = rng.standard_normal((R, 3 * e)).astype(np.float32)
    hist = rng.standard_normal((t, R, 2 * e)).astype(np.float32)  # k | v of row r's position j
    k = np.concatenate([hist[:, :, :e], qkv[None, :, e:2 * e]], 0).astype(np.float64)  # [t+1,R,e]
    v = np.concatenate([hist[:, :, e:], qkv[None, :, 2 * e:]], 0).astype(np.float64)
    q = qkv[:, :e].astype(np.float64)
    ref = np.zeros((R, e))
    for r in range(R):
        for h in range(H):
            sl = slice(h * dh, (h + 1) * dh)
            s = k[:, r, sl] @ q[r, sl] / math.sqrt(dh)
            p = np.exp(s - s.max())
            ref[r, sl] = (p / p.sum()) @ v[:, r, sl]
    for a in (qkv, hist, ref):
        a.setflags(write=False)
    return qkv, hist, ref


def _placed_cache(hist, R, L, e, seed, gpu):
    """The history stored under a random slot assignment (one permutation of the rows per
    position), every other cache entry NaN; -> (cache [L, R, 2e], anc int32 [R, L])."""
    t = hist.shape[0]
    rng = np.random.default_rng(seed)
    cache = np.full((L, R, 2 * e), np.nan, np.float32)
    anc = rng.integers(0, R, size=(R, L)).astype(np.int32)  # positions >= t: never read
    for j in range(t):
        perm = rng.permutation(R)
        anc[:, j] = perm
        cache[j, perm] = hist[j]
    return torch.from_numpy(cache).to(gpu), torch.from_numpy(anc).to(gpu)


@pytest.mark.parametrize("i", range(len(STEP_CASES)),
                         ids=["x".join(map(str, c)) for c in STEP_CASES])
def test_step_attention_matches_float64_and_honours_anc(gpu, i):
    from onebit_asr import _lib
    from onebit_asr.attdec import decattn_step

    R, H, dh, L, t = STEP_CASES[i]
    e = H * dh
    qkv, hist, ref = _step_case(i)
    d_qkv = torch.from_numpy(qkv).to(gpu)
    outs = []
    for seed in (1, 2):
        cache, anc = _placed_cache(hist, R, L, e, 7100 + 10 * i + seed, gpu)
        ctx = decattn_step(d_qkv, cache, anc, None, H, t)
        assert ctx.shape == (R, e) and torch.isfinite(ctx).all()
        # the rows' own k | v were appended at (t, r); nothing else was written
        assert torch.equal(_bits(cache[t]), _bits(d_qkv[:, e:]))
        assert torch.isnan(cache[t + 1:]).all()
        outs.append(ctx)
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    err = float(np.abs(outs[0].cpu().numpy().astype(np.float64) - ref).max())
    # the existing forward on the same data: the last query row over its t + 1 keys
    lib = _lib.load()
    assert lib.ob_decattn_supported(1, t + 1, dh)
    kv = torch.from_numpy(np.ascontiguousarray(
        np.concatenate([hist, qkv[None, :, e:]], 0).transpose(1, 0, 2))).to(gpu)  # [R, t+1, 2e]
    q = d_qkv[:, :e].contiguous()
    old = torch.empty(R, 1, e, device=gpu)
    probs = torch.empty(R, H, 1, t + 1, device=gpu)
    assert lib.ob_decattn_fwd(q.data_ptr(), e, kv.data_ptr(), 2 * e, kv.data_ptr() + 4 * e, 2 * e,
                              None, 0, R, H, 1, t + 1, dh, 0.0, None, 0, probs.data_ptr(),
                              old.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    e_old = float(np.abs(old.view(R, e).cpu().numpy().astype(np.float64) - ref).max())
    print(f"R={R} H={H} dh={dh} L={L} t={t}: err {err:.3e}, existing forward {e_old:.3e}, "
          f"bar {4 * e_old:.3e}")
    assert err <= 4 * e_old
    # skipped rows: nothing stored, ctx untouched
    if R > 1:
        cache, anc = _placed_cache(hist, R, L, e, 7190 + i, gpu)
        skip = torch.zeros(R, dtype=torch.uint8, device=gpu)
        skip[1] = 1
        ctx = torch.full((R, e), 7.0, device=gpu)
        st = torch.cuda.current_stream().cuda_stream
        assert lib.ob_decattn_step(d_qkv.data_ptr(), 3 * e, cache.data_ptr(), anc.data_ptr(),
                                   skip.data_ptr(), R, H, dh, L, t, ctx.data_ptr(), st) == 0
        assert (ctx[1] == 7.0).all() and torch.isnan(cache[t, 1]).all()
        keep = [r for r in range(R) if r != 1]
        assert torch.equal(_bits(ctx[keep]), _bits(outs[0][keep]))


# ------------------------------------------------------------------------------------------
# 2. the output layer with top-k
# ------------------------------------------------------------------------------------------
TOPK_R = [1, 17, 130]
TOPK_DV = [(16, 5), (64, 64), (64, 65), (256, 64), (144, 5004)]
TOPK_K = [1, 10, 32]
BANNED = (0, 1, 3)
GAP = 2e-3  # the construction's smallest float64 gap between neighbouring ranks (see below)


def _ranked(z, banned):
    """Candidate ids of a float64 logit row, best first (ties: the smaller id)."""
    ids = np.array([v for v in range(z.shape[0]) if v not in banned])
    return ids[np.lexsort((ids, -z[ids]))]


@functools.lru_cache(maxsize=None)
def _topk_case(R, d, V):
    """Rows are redrawn until the float64 reference has a gap of at least GAP x max(1, max|z|/80)
    between every pair of neighbours among its 33 best candidates (a property of the reference
    alone), except the engineered exact tie."""
    rng = np.random.default_rng(8000 + 131 * R + 7 * d + V)
    W = rng.standard_normal((V, d)).astype(np.float32)
    bias = rng.standard_normal(V).astype(np.float32)
    tie = None
    if V >= 64:
        tie = (V - 9, V - 5)     # two identical rows of the output layer
        W[tie[1]] = W[tie[0]]
        bias[tie[1]] = bias[tie[0]]
    W64, b64 = W.astype(np.float64), bias.astype(np.float64)

    def engineered(r):
        c = {0: V - 1, 1: BANNED[2], 2: tie[0] if tie else None}.get(r)
        if c is None:
            return None
        return W[c] * np.float32(60.0 / float((W64[c] ** 2).sum()))

    h = np.zeros((R, d), np.float32)
    for r in range(R):
        for _ in range(200):
            base = engineered(r)
            row = rng.standard_normal(d).astype(np.float32)
            row = row if base is None else base + np.float32(0.05) * row
            z = row.astype(np.float64) @ W64.T + b64
            top = z[_ranked(z, BANNED)][:33]
            gaps = top[:-1] - top[1:]
            if tie is not None:
                gaps = gaps[gaps != 0.0]  # (the identical rows: an exact tie, checked by index)
            if gaps.size == 0 or gaps.min() >= GAP * max(1.0, np.abs(z).max() / 80.0):
                break
        else:
            raise AssertionError("no row with clear gaps found")
        h[r] = row
    z = h.astype(np.float64) @ W64.T + b64
    m = z.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))[:, 0]
    order = [_ranked(z[r], BANNED) for r in range(R)]
    th, tW, tb = torch.from_numpy(h), torch.from_numpy(W), torch.from_numpy(bias)
    z32 = torch.nn.functional.linear(th, tW, tb)
    rows = np.arange(R)[:, None]
    rep = np.stack([np.resize(o[:32], 32) for o in order])    # the ids a call can report
    e_torch = max(float(np.abs(z32.numpy()[rows, rep] - z[rows, rep]).max()),
                  float(np.abs(torch.logsumexp(z32, dim=-1).numpy() - lse).max()))
    for a in (h, W, bias, z, lse):
        a.setflags(write=False)
    return h, W, bias, z, lse, order, e_torch, tie


@pytest.mark.parametrize("d,V", TOPK_DV, ids=[f"{d}x{V}" for d, V in TOPK_DV])
@pytest.mark.parametrize("R", TOPK_R)
def test_seq_topk_matches_float64(gpu, R, d, V):
    from onebit_asr.attdec import seq_topk

    h, W, bias, z, lse_ref, order, e_torch, tie = _topk_case(R, d, V)
    mx = float(np.abs(z).max())
    bar = max(1e-5 * mx, 4 * e_torch)
    dh, dW, db = (torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (h, W, bias))
    # the engineered rows are what they claim
    assert order[0][0] == V - 1 or V - 1 in BANNED or V <= 5
    if V == 5004:
        assert V % 64 == 12 and int(np.argmax(z[0])) == V - 1   # last column of the 12-wide tail
    if R > 1:
        assert int(np.argmax(z[1])) == BANNED[2]                 # the maximum is a banned id
    if R > 2 and tie is not None:
        assert list(order[2][:2]) == list(tie) and z[2, tie[0]] == z[2, tie[1]]
    skip = torch.zeros(R, dtype=torch.uint8, device=gpu)
    if R > 3:
        skip[3] = 1
        skip[R - 1] = 1
    if R >= 130:
        skip[64:128] = 1   # four whole subtiles without a live row
    live = (skip == 0).cpu().numpy()
    worst = 0.0
    for K in TOPK_K:
        out = (torch.full((R,), 77.0, dtype=torch.float64, device=gpu),
               torch.full((R, K), 77.0, device=gpu),
               torch.full((R, K), 77, dtype=torch.int32, device=gpu))
        lse, topv, topi = seq_topk(dh, dW, db, K, BANNED, skip if R > 3 else None, out)
        assert lse.dtype == torch.float64 and topv.dtype == torch.float32
        assert topi.dtype == torch.int32 and topv.shape == topi.shape == (R, K)
        g_lse, g_v, g_i = lse.cpu().numpy(), topv.cpu().numpy().astype(np.float64), topi.cpu().numpy()
        # skipped rows are left untouched
        assert (g_lse[~live] == 77.0).all() and (g_v[~live] == 77.0).all()
        assert (g_i[~live] == 77).all()
        err = float(np.abs(g_lse[live] - lse_ref[live]).max())
        for r in np.nonzero(live)[0]:
            n = min(K, len(order[r]))
            assert n < K or len(order[r]) >= K
            want = order[r][:n]
            err = max(err, float(np.abs(g_v[r, :n] - z[r, want]).max()))
            # padding when fewer than K candidates exist (V = 5: ids 2 and 4 only)
            assert (g_i[r, n:] == -1).all() and (g_v[r, n:] == NEG_INF).all()
        worst = max(worst, err)
        assert err <= bar, (K, err, bar)
        for r in np.nonzero(live)[0]:
            n = min(K, len(order[r]))
            full = z[r, order[r]]
            for q in range(n):
                gap = full[q] - full[q + 1] if q + 1 < len(full) else np.inf
                exact_tie = tie is not None and gap == 0.0 and \
                    (int(order[r][q]), int(order[r][q + 1])) == tie
                # nothing is silently left out: every reported rank is decided
                assert gap >= 10 * err or exact_tie, (r, q, gap, err)
            assert g_i[r, :n].tolist() == order[r][:n].tolist(), (K, r)
        again = seq_topk(dh, dW, db, K, BANNED, skip if R > 3 else None)
        for a, b_ in zip((lse, topv, topi), again):   # bitwise reproducible (live rows)
            assert a.cpu().numpy()[live].tobytes() == b_.cpu().numpy()[live].tobytes()
    print(f"R={R} d={d} V={V}: max|logit| {mx:.2f} err {worst:.3e} e_torch {e_torch:.3e} "
          f"bar {bar:.3e}")


def test_seq_topk_without_bias_ban_or_skip(gpu):
    from onebit_asr.attdec import seq_topk

    h, W, _, _, _, _, _, _ = _topk_case(17, 64, 65)
    z = h.astype(np.float64) @ W.astype(np.float64).T
    lse, topv, topi = seq_topk(torch.from_numpy(np.ascontiguousarray(h)).to(gpu),
                               torch.from_numpy(np.ascontiguousarray(W)).to(gpu), None, 3)
    m = z.max(axis=1)
    assert np.abs(lse.cpu().numpy() - (m + np.log(np.exp(z - m[:, None]).sum(axis=1)))).max() <= 1e-4
    assert topi[:, 0].cpu().tolist() == z.argmax(axis=1).tolist()


# ------------------------------------------------------------------------------------------
# 3. beam step / finalize against the oracle bookkeeping
# ------------------------------------------------------------------------------------------
def _hash_logp(seed, V, eos):
    """A deterministic per-prefix table of binary fractions (multiples of 1/64 in [-8, 0]):
    every float64 sum is exact and ties are frequent."""
    def logp(prefixes):
        out = []
        for p in prefixes:
            rng = np.random.default_rng(zlib.crc32(repr((seed, tuple(p))).encode()))
            lp = -rng.integers(0, 513, size=V).astype(np.float64) / 64.0
            if rng.random() < 0.3:
                lp[eos] = -rng.integers(0, 16) / 64.0
            out.append(lp)
        return out
    return logp


def _run_bookkeeping(gpu, logps, alive, N, L, alpha, special, V):
    """Drive init / beam_step / finalize with the top-N tables the oracle's own slots produce,
    and compare everything after every step."""
    from onebit_asr import _lib
    from onebit_asr.attdec import length_norm

    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    ids = dict(ar.SPECIAL, **(special or {}))
    banned = {ids["pad"], ids["bos"], ids["blank"]}
    B = len(logps)
    R = B * N
    refs = [ar.beam_search(lp, N, L, alpha, special, alive=a) for lp, a in zip(logps, alive)]
    hists = [ar.walk_trace([[p for p, _, _ in row] for row in r.trace],
                           [[v for _, v, _ in row] for row in r.trace],
                           [[s for _, _, s in row] for row in r.trace], N, ids["eos"], a)
             for r, a in zip(refs, alive)]
    kmask = torch.zeros(B, 3, dtype=torch.uint8, device=gpu)
    for b, a in enumerate(alive):
        if not a:
            kmask[b] = 1
    score = torch.full((B, N), 5.0, dtype=torch.float64, device=gpu)
    length = torch.full((B, N), 9, dtype=torch.int32, device=gpu)
    fin = torch.full((B, N), 9, dtype=torch.uint8, device=gpu)
    tok = torch.full((R,), 9, dtype=torch.int64, device=gpu)
    skip = torch.full((R,), 9, dtype=torch.uint8, device=gpu)
    anc = torch.full((2, R, L), -5, dtype=torch.int32, device=gpu)
    trp = torch.full((L, B, N), 9, dtype=torch.int32, device=gpu)
    trt = torch.full((L, B, N), 9, dtype=torch.int32, device=gpu)
    trs = torch.full((L, B, N), 9.0, dtype=torch.float64, device=gpu)
    norm = length_norm(L, alpha)
    assert norm.tolist() == ar.length_norm(L, alpha)
    norm = norm.to(gpu)
    assert lib.ob_attdec_init(kmask.data_ptr(), B, N, 3, L, ids["bos"], score.data_ptr(),
                              length.data_ptr(), fin.data_ptr(), tok.data_ptr(), skip.data_ptr(),
                              anc[0].data_ptr(), st) == 0
    assert tok.cpu().tolist() == [ids["bos"]] * R
    assert fin.cpu().tolist() == [[0 if (a and k == 0) else 2 for k in range(N)] for a in alive]
    for t in range(L):
        lse = np.full(R, np.nan)
        topv = np.full((R, N), np.nan, np.float32)
        topi = np.full((R, N), 12345, np.int32)     # rows that are not live hold rubbish
        for b in range(B):
            slots = hists[b][t]
            live = [k for k, s in enumerate(slots) if s is not None and not s.fin]
            assert skip.cpu().tolist()[b * N:(b + 1) * N] == [0 if k in live else 1
                                                              for k in range(N)]
            for k, lp in zip(live, logps[b]([slots[k].toks for k in live])):
                cand = np.array([v for v in range(V) if v not in banned])
                order = cand[np.lexsort((cand, -lp[cand]))][:N]
                shift = float(b + k)               # lse is honoured: logit = lp + lse
                lse[b * N + k] = shift
                topv[b * N + k, :len(order)] = (lp[order] + shift).astype(np.float32)
                topv[b * N + k, len(order):] = NEG_INF
                topi[b * N + k, :len(order)] = order
                topi[b * N + k, len(order):] = -1
        d_lse, d_v, d_i = (torch.from_numpy(a).to(gpu) for a in (lse, topv, topi))
        assert lib.ob_attdec_beam_step(
            d_lse.data_ptr(), d_v.data_ptr(), d_i.data_ptr(), B, N, N, L, t, ids["eos"],
            ids["pad"], norm.data_ptr(), anc[t & 1].data_ptr(), anc[(t + 1) & 1].data_ptr(),
            score.data_ptr(), length.data_ptr(), fin.data_ptr(), tok.data_ptr(), skip.data_ptr(),
            trp.data_ptr(), trt.data_ptr(), trs.data_ptr(), st) == 0
        for b in range(B):
            row = refs[b].trace[t]
            assert trp[t, b].cpu().tolist() == [p for p, _, _ in row], (t, b)
            assert trt[t, b].cpu().tolist() == [v for _, v, _ in row], (t, b)
            assert trs[t, b].cpu().tolist() == [s for _, _, s in row], (t, b)
            new = hists[b][t + 1]
            assert score[b].cpu().tolist() == [NEG_INF if s is None else s.score for s in new]
            assert length[b].cpu().tolist() == [0 if s is None else s.n for s in new]
            assert fin[b].cpu().tolist() == [2 if s is None else int(s.fin) for s in new]
            want_tok = [ids["pad"] if (s is None or s.fin) else row[k][1]
                        for k, s in enumerate(new)]
            assert tok[b * N:(b + 1) * N].cpu().tolist() == want_tok
            want_anc = ar.ancestry(refs[b].trace[:t + 1], N, L, b * N)
            got_anc = anc[(t + 1) & 1, b * N:(b + 1) * N, :t + 1].cpu().tolist()
            assert got_anc == [r_[:t + 1] for r_ in want_anc], (t, b)
    hyp = torch.full((B, N, L), 9, dtype=torch.int32, device=gpu)
    hyp_len = torch.full((B, N), 9, dtype=torch.int32, device=gpu)
    n_hyp = torch.full((B,), 9, dtype=torch.int32, device=gpu)
    out_sc = torch.full((B, N), 9.0, dtype=torch.float64, device=gpu)
    fin_out = torch.full((B, N), 9, dtype=torch.uint8, device=gpu)
    assert lib.ob_attdec_finalize(trp.data_ptr(), trt.data_ptr(), score.data_ptr(),
                                  length.data_ptr(), fin.data_ptr(), B, N, L, ids["eos"],
                                  hyp.data_ptr(), hyp_len.data_ptr(), n_hyp.data_ptr(),
                                  out_sc.data_ptr(), fin_out.data_ptr(), st) == 0
    for b, r in enumerate(refs):
        n = len(r.hyps)
        assert n_hyp[b].item() == n
        for k in range(N):
            m = hyp_len[b, k].item()
            assert (hyp[b, k, m:] == -1).all()
            if k < n:
                assert hyp[b, k, :m].cpu().tolist() == r.hyps[k]
                assert out_sc[b, k].item() == r.scores[k]
                assert bool(fin_out[b, k].item()) == r.finished[k]
            else:
                assert m == 0 and out_sc[b, k].item() == NEG_INF and fin_out[b, k].item() == 0
    return refs


@pytest.mark.parametrize("alpha", [0.0, 0.6])
@pytest.mark.parametrize("N", [1, 4, 10])
def test_beam_step_and_finalize_match_the_oracle(gpu, N, alpha):
    V, L = 12, 6
    logps = [_hash_logp(100 * N + u, V, 2) for u in range(4)]
    refs = _run_bookkeeping(gpu, logps, [True, True, False, True], N, L, alpha, None, V)
    assert refs[2].hyps == []                                   # the all-masked utterance
    if N == 10:
        assert min(r.margin for r in refs if r.hyps) == 0.0     # an exact tie was decided
    if N > 1:
        assert any(any(r.finished) and not all(r.finished) for r in refs)


def test_beam_step_and_finalize_on_the_golden_cases(gpu):
    import json
    from pathlib import Path

    golden = json.loads((Path(__file__).parent / "golden" / "attdec_bookkeeping.json").read_text())
    for c in golden["cases"]:
        refs = _run_bookkeeping(gpu, [ar.table_logp(c["table"], c["default"])], [True], c["N"],
                                c["L"], c["alpha"], golden["special"], 5)
        assert refs[0].hyps == c["hyps"] and refs[0].scores == c["scores"]


# ------------------------------------------------------------------------------------------
# 4. end to end, eager, on synthetic memory
# ------------------------------------------------------------------------------------------
LENS = (61, 20, 1)


@functools.lru_cache(maxsize=None)
def _decoder_model(V, d):
    from onebit_asr.conformer import ConformerASR
    from onebit_asr.data import CFG1

    torch.manual_seed(0)
    cfg = dict(CFG1) if d == 64 else dict(CFG1, enc_d_model=d, enc_layers=1)
    model = ConformerASR(80, V, **cfg).to("cuda:0").eval()
    return model, rr.double_model(model)


def _memory(seed, d, lens, gpu):
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(len(LENS), 61, d, generator=g)   # (the same draw with or without row 4)
    mask = torch.zeros(len(lens), 61, dtype=torch.long)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    if len(lens) > len(LENS):
        enc = torch.cat([enc, torch.randn(len(lens) - len(LENS), 61, d, generator=g)])
    return enc.to(gpu), mask.to(gpu)


def _existing_logp(model, enc_b, mask_b, bos=1):
    """The comparator: ``model.decode_logits`` on the GPU (fp32, existing code, no cache) on the
    growing prefixes, log-softmax in float64 on the host."""
    def logp(prefixes):
        n = len(prefixes)
        inp = torch.tensor([[bos] + list(p) for p in prefixes], dtype=torch.long,
                           device=enc_b.device)
        with torch.no_grad():
            z = model.decode_logits(enc_b[None].repeat(n, 1, 1), mask_b[None].repeat(n, 1), inp,
                                    torch.zeros(inp.shape, dtype=torch.bool, device=enc_b.device))
        return torch.log_softmax(z[:, -1].double().cpu(), dim=-1).numpy()
    return logp


def _teacher_forced(model, enc, mask, hyps, finished, N, L):
    """Scores of the returned hypotheses from the existing rescoring path: ``decoder.hidden`` on
    the shared memory + ``seq_logprob``; the eos term only where the hypothesis is finished."""
    from onebit_asr.infer import seq_logprob

    inp, tgt, pad, _ = rr.prepare(hyps, N, L)
    for b, utt in enumerate(hyps):
        for k, y in enumerate(utt):
            if not finished[b][k]:
                tgt[b * N + k][len(y)] = -1
    dev = enc.device
    dec = model.decoder
    h = dec.hidden(torch.tensor(inp, dtype=torch.long, device=dev), enc, mask,
                   torch.tensor(pad, dtype=torch.bool, device=dev), mem_group=N)
    lp = seq_logprob(h.reshape(-1, h.shape[-1]), dec.out.weight, dec.out.bias,
                     torch.tensor(tgt, dtype=torch.int32, device=dev).reshape(-1))
    lp = lp.double().cpu().numpy().reshape(len(hyps) * N, L + 1)
    return [[float(sum(lp[b * N + k, j] for j in range(len(y) + int(finished[b][k]))))
             for k, y in enumerate(utt)] for b, utt in enumerate(hyps)]


def _check_end_to_end(gpu, model, model64, enc, mask, N, L, alpha, tag, must_be_decisive=False):
    from onebit_asr.attdec import attention_beam_search

    B = enc.shape[0]
    hyp, hyp_len, n_hyp, score, info = attention_beam_search(model, enc, mask, N, L, alpha)
    assert hyp.shape == (B, N, L) and hyp.dtype == hyp_len.dtype == n_hyp.dtype == torch.int32
    assert score.dtype == torch.float64 and info["finished"].dtype == torch.bool
    assert info["trace_parent"].shape == info["trace_token"].shape == (L, B, N)
    h_, l_, n_, s_ = (t.cpu().numpy() for t in (hyp, hyp_len, n_hyp, score))
    f_ = info["finished"].cpu().numpy()
    tp, tt, ts = (info[k].cpu().numpy() for k in ("trace_parent", "trace_token", "trace_score"))
    enc64, mask_c = enc.cpu().numpy(), mask.cpu().numpy()
    hyps, fins, es = [], [], []
    for b in range(B):
        alive = bool(mask_c[b].any())
        got = [h_[b, k, :l_[b, k]].tolist() for k in range(n_[b])]
        hyps.append(got)
        fins.append([bool(f_[b, k]) for k in range(n_[b])])
        for k in range(N):
            assert (h_[b, k, l_[b, k]:] == -1).all()
            if k >= n_[b]:
                assert l_[b, k] == 0 and s_[b, k] == NEG_INF and not f_[b, k]
        if not alive:
            assert n_[b] == 0 and (tt[:, b] == ar.DEAD).all()
            es.append(0.0)
            continue
        logp64 = ar.model_logp(model64, enc64[b], mask_c[b])
        e, worst, last = ar.check_search(tp[:, b], tt[:, b], ts[:, b], logp64,
                                         _existing_logp(model, enc[b], mask[b]), N, L, alpha)
        es.append(e)
        # what finalize returned is what the trace says
        live = [s for s in last if s is not None]
        assert got == [s.toks for s in live] and fins[b] == [s.fin for s in live]
        assert s_[b, :n_[b]].tolist() == [s.score for s in live]
        ref = ar.beam_search(logp64, N, L, alpha)
        decisive = ref.margin >= 10 * e
        print(f"{tag} utt {b}: e {e:.3e} device score err {worst:.3e} oracle margin "
              f"{ref.margin:.3e} decisive {decisive} finished {sum(fins[b])}/{n_[b]}")
        if must_be_decisive:
            assert decisive, (b, ref.margin, e)
        if decisive:
            assert got == ref.hyps and fins[b] == ref.finished, (b, got, ref.hyps)
            assert max(abs(a - c) for a, c in zip(s_[b], ref.scores)) <= e
    tf = _teacher_forced(model, enc, mask, hyps, fins, N, L)
    for b in range(B):
        for k in range(n_[b]):
            assert abs(s_[b, k] - tf[b][k]) <= es[b], (b, k, s_[b, k], tf[b][k], es[b])
    return hyps, fins


E2E_CASES = [(V, N, L) for V in (40, 5004) for N, L in ((1, 12), (4, 8), (10, 12))]


@pytest.mark.parametrize("V,N,L", E2E_CASES, ids=[f"V{V}-N{N}-L{L}" for V, N, L in E2E_CASES])
def test_attention_search_end_to_end(gpu, V, N, L):
    model, model64 = _decoder_model(V, 64)
    lens = LENS + (0,) if (V, N) == (40, 4) else LENS   # one case with an all-masked row
    enc, mask = _memory(0, 64, lens, gpu)
    _check_end_to_end(gpu, model, model64, enc, mask, N, L, 0.0, f"V={V} N={N} L={L}",
                      must_be_decisive=(V == 40 and N == 1))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_greedy_search_is_decisive_and_exact(gpu, seed):
    model, model64 = _decoder_model(40, 64)
    enc, mask = _memory(seed, 64, LENS, gpu)
    _check_end_to_end(gpu, model, model64, enc, mask, 1, 12, 0.0, f"greedy seed {seed}",
                      must_be_decisive=True)


@pytest.mark.parametrize("N,L,alpha", [(4, 8, 0.0), (10, 12, 0.6)])
def test_attention_search_d144(gpu, N, L, alpha):
    model, model64 = _decoder_model(40, 144)      # d = 144, H = 4: dh = 36
    enc, mask = _memory(0, 144, LENS, gpu)
    _check_end_to_end(gpu, model, model64, enc, mask, N, L, alpha, f"d=144 N={N} alpha={alpha}")


def test_attention_search_with_eos(gpu):
    """decoder.out.bias[eos] + 0.75 (tuned on the CPU oracle): at least one hypothesis finishes
    before step L - 1 and at least one is still unfinished after L."""
    base, _ = _decoder_model(40, 64)
    model = copy.deepcopy(base)
    with torch.no_grad():
        model.decoder.out.bias[2] += 0.75
    model64 = rr.double_model(model)
    N, L = 4, 8
    enc, mask = _memory(0, 64, LENS, gpu)
    enc64, mask_c = enc.cpu().numpy(), mask.cpu().numpy()
    refs = [ar.beam_search(ar.model_logp(model64, enc64[b], mask_c[b]), N, L) for b in range(3)]
    early = sum(f and len(h) < L - 1 for r in refs for h, f in zip(r.hyps, r.finished))
    unfinished = sum(not f for r in refs for f in r.finished)
    assert early >= 1 and unfinished >= 1
    for alpha in (0.0, 0.6):
        hyps, fins = _check_end_to_end(gpu, model, model64, enc, mask, N, L, alpha,
                                       f"eos alpha={alpha}")
        assert any(f for u in fins for f in u) and any(not f for u in fins for f in u)


def test_attention_decode_batch_and_switch(gpu):
    from onebit_asr.attdec import attention_beam_search
    from onebit_asr.metrics import attention_decode_batch

    model, _ = _decoder_model(40, 64)
    enc, mask = _memory(0, 64, LENS, gpu)
    hyp, hyp_len, _, _, _ = attention_beam_search(model, enc, mask, 4, 8)
    got = attention_decode_batch(model, enc, mask, beam_size=4, max_len=8)
    assert got == [hyp[b, 0, :hyp_len[b, 0]].tolist() for b in range(3)]
    with pytest.raises(ValueError, match="not supported"):
        attention_beam_search(model, enc, mask, 33, 8)
    with pytest.raises(ValueError, match="not supported"):
        attention_beam_search(model, enc, mask, 4, 256)


# ------------------------------------------------------------------------------------------
# 5. graphed
# ------------------------------------------------------------------------------------------
def test_graphed_attention_search_equals_eager_bitwise(gpu):
    from onebit_asr.conformer import ConformerASR
    from onebit_asr.data import CFG1, synthetic_batch
    from onebit_asr.infer import GraphedInference, encode_and_decode
    from onebit_asr.quant import set_act_quant

    torch.manual_seed(0)
    model = ConformerASR(80, 5004, **CFG1).to(gpu).eval()
    feat_lens, tok_lens = [349, 61], [12, 3]
    b1 = synthetic_batch(feat_lens, tok_lens, seed=0, device=gpu)
    b2 = synthetic_batch(feat_lens, tok_lens, seed=1, device=gpu)
    gi = GraphedInference(model, act_quant=None, decoder="attention", beam_size=4, max_len=12)
    keys = ("hyp", "hyp_len", "n_hyp", "score", "finished", "trace_parent", "trace_token",
            "trace_score")
    runs = []
    for b in (b1, b1, b2, b1):
        out, cnt, _ = gi.run(b)
        runs.append((out.clone(), cnt.clone(), {k: gi.info[k].clone() for k in keys}))
    assert gi.graph is not None
    set_act_quant(model, None)
    eager = []
    for b in (b1, b2):
        info = {}
        out, cnt, _ = encode_and_decode(model, b, decoder="attention", beam_size=4, max_len=12,
                                        info=info)
        assert out.shape == (2, 12) and out.dtype == cnt.dtype == torch.int32
        assert torch.equal(out, info["hyp"][:, 0]) and torch.equal(cnt, info["hyp_len"][:, 0])
        eager.append((out, cnt, info))

    def same(run, ref):
        assert torch.equal(run[0], ref[0]) and torch.equal(run[1], ref[1])
        for k in keys:
            assert run[2][k].cpu().numpy().tobytes() == ref[2][k].cpu().numpy().tobytes(), k

    same(runs[0], eager[0])      # the first run equals eager, bit for bit
    same(runs[1], runs[0])       # two replays of the same batch
    same(runs[3], runs[0])
    same(runs[2], eager[1])      # another batch of the same shape: that batch's eager result
