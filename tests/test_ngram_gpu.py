"""GPU: n-gram LM shallow fusion (csrc/ngram.hip, the fused step of csrc/attdec.hip, the LM pick
of csrc/rescore.hip, ``onebit_asr.ngram``) against the oracle of tests/ngram_ref.py.

Bars.
* ``ob_ngram_step`` / ``ob_ngram_seq_logprob``: equal bits to the dict oracle (the rule's float64
  sum of float32 table values has one order); the same bits under a permuted slot assignment;
  skipped rows keep a poison value in ``lmsc`` and ``ctx_out``; absent candidates are -inf.
* Fused step / finalize: equal to the oracle bookkeeping exactly (binary fractions).
* End to end: ``ngram_ref.check_fused_search``, the joint search's step-wise rule with the LM term
  (exact, so e is unchanged: 4x the error of the existing attention path + 1e-9 * max(1, T));
  where the oracle's smallest margin is >= 10e the n-best, finished, S, A, C and Lm equal the
  oracle's. Every N = 1 case must be decisive.
* Forcing: an LM that puts almost all mass on one chain, at weight 50, makes the joint search and
  the LM-rescored CTC n-best return exactly that chain; without the LM they do not.
* No-op: ``lm=None`` and ``lm_weight == 0`` are bitwise the call without the keywords, in every
  decoder. ``ob_rescore_select_lm``: total and best_k equal the float64 formula exactly.
* Graphed: bitwise equal to eager, replays bitwise equal.

Figures seen on an MI355X (each test prints its own, -s; log profiles/r10/ngram_gpu_tests.log):
4547 step scores and 48 hypothesis rows equal to the oracle's bits, every outcome class covered
(hit at orders 1..4, full back-off, a context that is no entry, unknown token, short prefix, absent
candidate, skipped row); end to end e is 3.9e-7 to 2.4e-6, the device S error at most 8.4e-7, the
oracle margins 9.4e-5 (N = 10, w = 0.3, T = 20) to 8.8e-2, N = 1 at least 3.5e-4: every case
decisive and equal to the oracle's n-best; the T = 1 utterance drops 31 / 93 / 279 candidates
(N = 1 / 4 / 10) when w > 0.
"""
import functools
import math

import numpy as np
import pytest
import torch

import attdec_ref as ar
import joint_ref as jr
import ngram_ref as nr
import test_joint_gpu as tj

pytestmark = pytest.mark.gpu

NEG_INF = -math.inf
PAD, BOS, EOS, BLANK = 0, 1, 2, 3
POISON = 77


def _bytes(t):
    return t.cpu().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def _lm(order, V):
    """(NGramLM, RefLM) of a case: the shared 2e5-entry table at V = 5004, small random ones else."""
    from onebit_asr.ngram import NGramLM

    if V == 5004:
        ref, ids, n, vals = nr.big_lm()
        assert order == ref.order
    else:
        entries, ids, n, vals = nr.random_lm(500 + V, order, V, {5: 3, 9: 20, 35: 400}[V])
        ref = nr.RefLM(entries, order)
    return NGramLM.from_arrays(ids, n, vals, order), ref


# ------------------------------------------------------------------------------------------
# 1. the step scorer alone, along oracle-chosen prefix trees
# ------------------------------------------------------------------------------------------
#              B  N   K  order V
STEP_CASES = [(1, 1, 1, 1, 5), (2, 3, 5, 2, 9), (3, 10, 32, 3, 35), (2, 4, 20, 4, 5004)]
STEP_STEPS = 4


@functools.lru_cache(maxsize=None)
def _step_plan(i):
    """The logical tree of a case: per step and utterance N nodes (parent node, token appended, the
    K candidates to score, skipped) with the oracle's scores, and the outcomes the case covers."""
    B, N, K, order, V = STEP_CASES[i]
    _, ref = _lm(order, V)
    rng = np.random.default_rng(9300 + i)
    usable = [v for v in range(V) if v not in (PAD, BOS, BLANK, EOS)]
    follow = {}                                     # context -> the words that continue it
    for g in ref.entries:
        follow.setdefault(g[:-1], []).append(g[-1])
    # node 0 of every utterance walks one of the table's own 4-grams: a hit at the full order
    forced = next((g for g in ref.entries if len(g) == 4 and all(v in usable for v in g)), None)
    cover = set()
    steps, prev = [], None
    for s in range(STEP_STEPS):
        nodes = []
        for b in range(B):
            for j in range(N):
                if s == 0:
                    par, tok, toks = -1, -1, []
                else:
                    choices = [q for q in range(N) if not prev[b * N + q]["skip"]]
                    par = int(rng.choice(choices))
                    pn = prev[b * N + par]
                    real = [int(c) for c in pn["cand"] if c >= 0 and c != EOS] or usable
                    known = [c for c in pn["cand"][:pn["known"]] if c >= 0 and c != EOS]
                    # (mostly along the table's own n-grams, so that long hits occur)
                    tok = int(rng.choice(known if known and rng.random() < 0.7 else real))
                    if forced and j == 0:
                        par, pn, tok = 0, prev[b * N], forced[s - 1]
                    toks = pn["toks"] + [tok]
                h = ref.context(toks)
                cand = []
                for m in range(len(h), -1, -1):     # words the table knows after the context
                    for c in follow.get(tuple(h[len(h) - m:]), [])[:2]:
                        if c not in cand and c not in (PAD, BOS, BLANK) and len(cand) < K - 1:
                            cand.append(int(c))
                known = len(cand)
                for c in rng.permutation(usable):
                    if len(cand) >= K:
                        break
                    if int(c) not in cand:
                        cand.append(int(c))
                cand += [-1] * (K - len(cand))
                if forced and j == 0 and toks == list(forced[:s]):
                    cand[0] = forced[s]
                if K >= 2 and j % 3 != 2:
                    cand[1] = EOS
                if K >= 3:
                    cand[K - 1] = -1
                skip = N > 1 and s == 2 and b == B - 1 and j == N - 1
                if skip:
                    cover.add("skip")
                want = []
                for c in cand:
                    val, tags = ref.score_detail(toks, c)
                    want.append(val)
                    cover |= tags
                nodes.append(dict(par=par, tok=tok, toks=toks, cand=cand, skip=skip, want=want,
                                  known=known))
        steps.append(nodes)
        prev = nodes
    return steps, cover


def _drive_step(gpu, i, seed):
    """Run the plan with a random slot placement per step (seed None: the identity); returns per
    step (lmsc [R, K], ctx_out [R]) in LOGICAL node order."""
    from onebit_asr.ngram import ngram_step

    B, N, K, order, V = STEP_CASES[i]
    R = B * N
    lm, _ = _lm(order, V)
    steps, _ = _step_plan(i)
    rng = np.random.default_rng(seed) if seed is not None else None
    ctx = torch.full((2, R), POISON, dtype=torch.int64, device=gpu)
    place_prev = None
    out = []
    for s, nodes in enumerate(steps):
        place = np.arange(R)
        if rng is not None:
            for b in range(B):
                place[b * N:(b + 1) * N] = b * N + rng.permutation(N)
        topi = np.zeros((R, K), np.int32)
        tok = np.full(R, BOS, np.int64)
        length = np.full(R, s, np.int32)
        link = np.full((R, 2), -7, np.int32)        # (rubbish where it must not be read)
        skip = np.zeros(R, np.uint8)
        for q, nd in enumerate(nodes):
            r, b = place[q], q // N
            topi[r] = nd["cand"]
            skip[r] = nd["skip"]
            if s > 0:
                tok[r] = nd["tok"]
                pq = b * N + nd["par"]
                ptoks = steps[s - 1][pq]["toks"]
                link[r] = (place_prev[pq], ptoks[-1] if ptoks else -1)
        lmsc = torch.full((R, K), float(POISON), dtype=torch.float64, device=gpu)
        c_out = ctx[(s + 1) & 1]
        c_out.fill_(POISON)
        ngram_step(lm, torch.from_numpy(topi).to(gpu), torch.from_numpy(tok).to(gpu),
                   torch.from_numpy(length).to(gpu), torch.from_numpy(link).to(gpu),
                   torch.from_numpy(skip).to(gpu), ctx[s & 1], c_out, lmsc, N, V)
        idx = torch.from_numpy(place).to(gpu)
        out.append((lmsc[idx].cpu().numpy(), c_out[idx].cpu().numpy()))
        place_prev = place
    return out


@pytest.mark.parametrize("i", range(len(STEP_CASES)),
                         ids=["x".join(map(str, c)) for c in STEP_CASES])
def test_ngram_step_equals_the_oracle_bit_for_bit(gpu, i):
    B, N, K, order, V = STEP_CASES[i]
    lm, _ = _lm(order, V)
    steps, cover = _step_plan(i)
    runs = [_drive_step(gpu, i, seed) for seed in (None, 1, 2)]
    n_inf = n_scored = 0
    for s, nodes in enumerate(steps):
        lmsc, ctx = runs[0][s]
        for other in runs[1:]:                       # the same bits wherever the prefix sits
            assert other[s][0].tobytes() == lmsc.tobytes(), s
            assert other[s][1].tobytes() == ctx.tobytes(), s
        assert not np.isnan(lmsc).any()
        for q, nd in enumerate(nodes):
            if nd["skip"]:
                assert (lmsc[q] == POISON).all() and ctx[q] == POISON
                continue
            assert int(ctx[q]) == lm.context(nd["toks"]), (s, q)
            for c, got, want in zip(nd["cand"], lmsc[q], nd["want"]):
                assert got == want, (s, q, c, got, want)         # equal bits; -inf exactly
                n_inf += want == NEG_INF
                n_scored += 1
                assert (c < 0) == (got == NEG_INF)               # the absent-candidate convention
    print(f"B={B} N={N} K={K} order={order} V={V}: {n_scored} scores equal, {n_inf} absent; "
          f"covers {sorted(cover)}")


def test_step_cases_cover_every_outcome():
    cover = set()
    for i in range(len(STEP_CASES)):
        cover |= _step_plan(i)[1]
    assert cover >= {"hit1", "hit2", "hit3", "hit4", "backoff_full", "ctx_missing", "unk", "short",
                     "absent", "skip"}, cover


# ------------------------------------------------------------------------------------------
# 2. whole-hypothesis scores
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 7, 61])
def test_ngram_seq_logprob_equals_the_oracle_bit_for_bit(gpu, T):
    from onebit_asr.ngram import ngram_seq_logprob

    V = 5004
    lm, ref = _lm(4, V)
    rng = np.random.default_rng(9400 + T)
    grams = [g for g in ref.entries if len(g) == 4 and BOS not in g and EOS not in g]
    lens = [0, T, -1, T, max(T - 1, 0), -3] + [int(v) for v in rng.integers(0, T + 1, size=10)]
    hyp = np.full((len(lens), T), -1, np.int32)
    for r, n in enumerate(lens):
        toks = []
        while len(toks) < max(n, 0):                 # chains of the table's own 4-grams and noise
            toks += list(grams[int(rng.integers(len(grams)))]) if rng.random() < 0.7 else \
                [int(rng.integers(4, V))]
        hyp[r, :max(n, 0)] = toks[:max(n, 0)]
    got, per_tok = ngram_seq_logprob(lm, torch.from_numpy(hyp).to(gpu),
                                     torch.tensor(lens, dtype=torch.int32), V, per_token=True)
    only = ngram_seq_logprob(lm, torch.from_numpy(hyp).to(gpu).view(2, -1, T),
                             torch.tensor(lens, dtype=torch.int32).view(2, -1), V)
    assert only.shape == (2, len(lens) // 2) and _bytes(only) == _bytes(got)
    got, per_tok = got.cpu().numpy(), per_tok.cpu().numpy()
    assert per_tok.shape == (len(lens), T + 1)
    for r, n in enumerate(lens):
        if n < 0:
            assert got[r] == NEG_INF and (per_tok[r] == 0).all()      # an absent row
            continue
        toks = hyp[r, :n].tolist()
        want = ref.seq_scores(toks)
        assert per_tok[r, :n + 1].tolist() == want, r
        assert (per_tok[r, n + 1:] == 0).all()
        total = 0.0
        for v in per_tok[r, :n + 1]:
            total += float(v)                        # per-token output sums to the total
        assert got[r] == total == ref.seq_logprob(toks), (r, got[r], total)
    print(f"T={T}: {len(lens)} rows equal (lengths {sorted(set(lens))})")


# ------------------------------------------------------------------------------------------
# 3. the fused beam step / finalize against the oracle bookkeeping
# ------------------------------------------------------------------------------------------
class _HashLM:
    """Lm increments of (prefix, token): multiples of 1/64 in [-8, 0] (exact sums)."""

    def __init__(self, seed):
        self.seed = seed

    def score(self, toks, v):
        import zlib

        return -float(zlib.crc32(repr(("lm", self.seed, tuple(toks), int(v))).encode()) % 513) / 64.0


def _run_fused_bookkeeping(gpu, logps, cscores, lms, alive, N, K, L, w, lw, alpha, V):
    from onebit_asr import _lib
    from onebit_asr.attdec import length_norm

    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    banned = {PAD, BOS, BLANK}
    B = len(logps)
    R = B * N
    x0 = np.zeros((1, V))
    refs = [nr.fused_search(lp, x0, lm, N, K, L, w, lw, alpha, alive=a,
                            cscore=cs if w > 0 else None)
            for lp, cs, lm, a in zip(logps, cscores, lms, alive)]
    kmask = torch.zeros(B, 3, dtype=torch.uint8, device=gpu)
    for b, a in enumerate(alive):
        if not a:
            kmask[b] = 1
    f64 = torch.float64
    score = torch.full((B, N), 5.0, dtype=f64, device=gpu)
    att = torch.zeros((B, N), dtype=f64, device=gpu)
    ctc = torch.zeros((B, N), dtype=f64, device=gpu)
    lmst = torch.zeros((B, N), dtype=f64, device=gpu)
    length = torch.full((B, N), 9, dtype=torch.int32, device=gpu)
    fin = torch.full((B, N), 9, dtype=torch.uint8, device=gpu)
    tok = torch.full((R,), 9, dtype=torch.int64, device=gpu)
    skip = torch.full((R,), 9, dtype=torch.uint8, device=gpu)
    link = torch.full((R, 2), 9, dtype=torch.int32, device=gpu)
    anc = torch.full((2, R, L), -5, dtype=torch.int32, device=gpu)
    trp = torch.full((L, B, N), 9, dtype=torch.int32, device=gpu)
    trt = torch.full((L, B, N), 9, dtype=torch.int32, device=gpu)
    trs = torch.full((L, B, N), 9.0, dtype=f64, device=gpu)
    norm = length_norm(L, alpha).to(gpu)
    assert lib.ob_attdec_init(kmask.data_ptr(), B, N, 3, L, BOS, score.data_ptr(),
                              length.data_ptr(), fin.data_ptr(), tok.data_ptr(), skip.data_ptr(),
                              anc[0].data_ptr(), st) == 0
    for t in range(L):
        lse = np.full(R, np.nan)
        topv = np.full((R, K), np.nan, np.float32)
        topi = np.full((R, K), 12345, np.int32)
        cpsi = np.full((R, K), np.nan)
        lmsc = np.full((R, K), np.nan)
        for b in range(B):
            slots = refs[b].history[t]
            live = [k for k, s in enumerate(slots) if s is not None and not s.fin]
            for k, lp in zip(live, logps[b]([slots[k].toks for k in live])):
                order = jr.top_candidates(lp, banned, K)
                shift = float(b + k)
                r = b * N + k
                lse[r] = shift
                topv[r, :len(order)] = (lp[order] + shift).astype(np.float32)
                topv[r, len(order):] = NEG_INF
                topi[r, :len(order)] = order
                topi[r, len(order):] = -1
                cpsi[r, :len(order)] = [cscores[b](slots[k].toks, v) for v in order]
                cpsi[r, len(order):] = NEG_INF
                lmsc[r, :len(order)] = [lms[b].score(slots[k].toks, v) for v in order]
                lmsc[r, len(order):] = NEG_INF
        d_lse, d_v, d_i, d_c, d_l = (torch.from_numpy(a).to(gpu)
                                     for a in (lse, topv, topi, cpsi, lmsc))
        assert lib.ob_attdec_fused_step(
            d_lse.data_ptr(), d_v.data_ptr(), d_i.data_ptr(), d_c.data_ptr() if w > 0 else None, w,
            d_l.data_ptr(), lw, B, N, K, L, t, EOS, PAD, norm.data_ptr(), anc[t & 1].data_ptr(),
            anc[(t + 1) & 1].data_ptr(), score.data_ptr(), att.data_ptr(), ctc.data_ptr(),
            lmst.data_ptr(), length.data_ptr(), fin.data_ptr(), tok.data_ptr(), skip.data_ptr(),
            link.data_ptr(), trp.data_ptr(), trt.data_ptr(), trs.data_ptr(), st) == 0
        for b in range(B):
            row = refs[b].trace[t]
            old, new = refs[b].history[t], refs[b].history[t + 1]
            assert trp[t, b].cpu().tolist() == [p for p, _, _ in row], (t, b)
            assert trt[t, b].cpu().tolist() == [v for _, v, _ in row], (t, b)
            assert trs[t, b].cpu().tolist() == [s for _, _, s in row], (t, b)
            inf_or = lambda f: [NEG_INF if s is None else f(s) for s in new]  # noqa: E731
            assert score[b].cpu().tolist() == inf_or(lambda s: s.S)
            assert att[b].cpu().tolist() == inf_or(lambda s: s.A)
            assert ctc[b].cpu().tolist() == inf_or(lambda s: s.C)
            assert lmst[b].cpu().tolist() == inf_or(lambda s: s.Lm)
            assert length[b].cpu().tolist() == [0 if s is None else s.n for s in new]
            assert fin[b].cpu().tolist() == [2 if s is None else int(s.fin) for s in new]
            want_tok = [PAD if (s is None or s.fin) else row[k][1] for k, s in enumerate(new)]
            assert tok[b * N:(b + 1) * N].cpu().tolist() == want_tok
            assert skip[b * N:(b + 1) * N].cpu().tolist() == [0 if (s is not None and not s.fin)
                                                              else 1 for s in new]
            want_link = []
            for k, (p, v, _) in enumerate(row):
                if v >= 0:
                    want_link.append([b * N + p, old[p].toks[-1] if old[p].toks else -1])
                else:
                    want_link.append([b * N + (k if p < 0 else p), -1])
            assert link[b * N:(b + 1) * N].cpu().tolist() == want_link, (t, b)
            want_anc = ar.ancestry(refs[b].trace[:t + 1], N, L, b * N)
            got_anc = anc[(t + 1) & 1, b * N:(b + 1) * N, :t + 1].cpu().tolist()
            assert got_anc == [r_[:t + 1] for r_ in want_anc], (t, b)
    hyp = torch.full((B, N, L), 9, dtype=torch.int32, device=gpu)
    hyp_len = torch.full((B, N), 9, dtype=torch.int32, device=gpu)
    n_hyp = torch.full((B,), 9, dtype=torch.int32, device=gpu)
    out_sc = torch.full((B, N), 9.0, dtype=f64, device=gpu)
    fin_out = torch.full((B, N), 9, dtype=torch.uint8, device=gpu)
    assert lib.ob_attdec_finalize(trp.data_ptr(), trt.data_ptr(), score.data_ptr(),
                                  length.data_ptr(), fin.data_ptr(), B, N, L, EOS,
                                  hyp.data_ptr(), hyp_len.data_ptr(), n_hyp.data_ptr(),
                                  out_sc.data_ptr(), fin_out.data_ptr(), st) == 0
    for b, r in enumerate(refs):
        n = len(r.hyps)
        assert n_hyp[b].item() == n
        for k in range(n):
            m = hyp_len[b, k].item()
            assert hyp[b, k, :m].cpu().tolist() == r.hyps[k]
            assert out_sc[b, k].item() == r.scores[k]
            assert bool(fin_out[b, k].item()) == r.finished[k]
    return refs


@pytest.mark.parametrize("alpha", [0.0, 0.6])
@pytest.mark.parametrize("w,lw", [(0.0, 0.5), (0.25, 0.5), (0.5, 2.0)])
@pytest.mark.parametrize("N,K", [(1, 1), (4, 8), (10, 20)])
def test_fused_step_and_finalize_match_the_oracle(gpu, N, K, w, lw, alpha):
    V, L = 40, 6
    logps = [jr.hash_logp(100 * N + u, V, EOS) for u in range(4)]
    cs = [tj._hash_cscore(7 * N + u) for u in range(4)]
    lms = [_HashLM(3 * N + u) for u in range(4)]
    refs = _run_fused_bookkeeping(gpu, logps, cs, lms, [True, True, False, True], N, K, L, w, lw,
                                  alpha, V)
    assert refs[2].hyps == []
    assert (sum(r.dropped for r in refs) > 0) == (w > 0)
    plain = [jr.joint_search(lp, np.zeros((1, V)), N, K, L, w, alpha, alive=a,
                             cscore=c if w > 0 else None)
             for lp, c, a in zip(logps, cs, [True, True, False, True])]
    assert [r.hyps for r in plain] != [r.hyps for r in refs] or N == 1   # the LM term matters


# ------------------------------------------------------------------------------------------
# 4. end to end, eager, on synthetic memory
# ------------------------------------------------------------------------------------------
def _check_fused(gpu, model, model64, enc, mask, lm, ref_lm, N, L, K, w, lw, tag,
                 decisive_utts=()):
    from onebit_asr.attdec import joint_beam_search

    B = enc.shape[0]
    with torch.no_grad():
        z = model.ctc_logits(enc).float().contiguous()
    hyp, hyp_len, n_hyp, score, info = joint_beam_search(model, enc, mask, z, N, L, w, K, 0.0,
                                                         lm=lm, lm_weight=lw)
    assert hyp.shape == (B, N, L) and score.dtype == torch.float64
    assert info["lm"].shape == info["att"].shape == (B, N) and info["lm"].dtype == torch.float64
    h_, l_, n_, s_ = (t.cpu().numpy() for t in (hyp, hyp_len, n_hyp, score))
    a_, c_, m_, f_ = (info[k].cpu().numpy() for k in ("att", "ctc", "lm", "finished"))
    tp, tt, ts = (info[k].cpu().numpy() for k in ("trace_parent", "trace_token", "trace_score"))
    for arr in (s_, a_, c_, m_, ts):
        assert not np.isnan(arr).any()
    enc64, mask_c, z_c = enc.cpu().numpy(), mask.cpu().numpy(), z.cpu().numpy()
    for b in range(B):
        T = int(mask_c[b].sum())
        got = [h_[b, k, :l_[b, k]].tolist() for k in range(n_[b])]
        fins = [bool(f_[b, k]) for k in range(n_[b])]
        for k in range(N):
            assert (h_[b, k, l_[b, k]:] == -1).all()
            if k >= n_[b]:
                assert l_[b, k] == 0 and not f_[b, k]
                assert s_[b, k] == a_[b, k] == c_[b, k] == m_[b, k] == NEG_INF
        x = jr.log_softmax64(z_c[b, :T])
        logp64 = tj._memo(ar.model_logp(model64, enc64[b], mask_c[b]))
        e, worst, final, last, dropped = nr.check_fused_search(
            tp[:, b], tt[:, b], ts[:, b], logp64, tj._existing_logp(model, enc[b], mask[b]), x,
            ref_lm, N, K, L, w, lw)
        live = [(s, fc) for s, fc in zip(last, final) if s is not None]
        assert got == [s.toks for s, _ in live] and fins == [s.fin for s, _ in live]
        assert s_[b, :n_[b]].tolist() == [s.score for s, _ in live]
        for k, (s, (oa, oc, ol)) in enumerate(live):    # A / C / Lm along the device's own path
            assert abs(a_[b, k] - oa) <= e and abs(c_[b, k] - oc) <= e, (b, k)
            assert m_[b, k] == ol, (b, k, m_[b, k], ol)                  # the LM term is exact
            assert s_[b, k] == nr.fuse(w, lw, a_[b, k], c_[b, k], m_[b, k])
            assert m_[b, k] == ref_lm.seq_logprob(s.toks) if s.fin else True
        ref = nr.fused_search(logp64, x, ref_lm, N, K, L, w, lw)
        decisive = ref.margin >= 10 * e
        print(f"{tag} utt {b} (T={T}): e {e:.3e} device S err {worst:.3e} oracle margin "
              f"{ref.margin:.3e} decisive {decisive} finished {sum(fins)}/{n_[b]} "
              f"dropped {dropped} (oracle search {ref.dropped})")
        if b in decisive_utts:
            assert decisive, (b, ref.margin, e)
        if decisive:
            assert got == ref.hyps and fins == ref.finished, (b, got, ref.hyps)
            for k in range(n_[b]):
                assert abs(s_[b, k] - ref.scores[k]) <= e
                assert abs(a_[b, k] - ref.att[k]) <= e and abs(c_[b, k] - ref.ctc[k]) <= e
                assert m_[b, k] == ref.lm[k]


E2E = [(N, L, w) for N, L in ((1, 12), (4, 8), (10, 12)) for w in (0.0, 0.3)]


@pytest.mark.parametrize("N,L,w", E2E, ids=[f"N{N}-L{L}-w{w}" for N, L, w in E2E])
def test_fused_search_end_to_end_v35(gpu, N, L, w):
    """V = 35, T' in {61, 20, 1}: 32 unbanned ids, so K = 32 takes the pre-beam out."""
    model, model64 = tj._decoder_model(35, 64)
    enc, mask = tj._memory(0, 64, tj.LENS, gpu)
    lm, ref_lm = _lm(3, 35)
    _check_fused(gpu, model, model64, enc, mask, lm, ref_lm, N, L, 32, w, 0.5,
                 f"V=35 N={N} L={L} w={w} lw=0.5", decisive_utts=(0, 1, 2) if N == 1 else ())


# ------------------------------------------------------------------------------------------
# 5. forcing
# ------------------------------------------------------------------------------------------
CHAIN = [9, 17, 5, 30, 12, 21]


def _chain_lm(V):
    from onebit_asr.ngram import NGramLM

    e = {(v,): (-20.0, 0.0) for v in range(V) if v not in (PAD, BLANK)}
    for a, b in zip([BOS] + CHAIN, CHAIN + [EOS]):
        e[(a, b)] = (-0.001, 0.0)
    return NGramLM(e, 2)


@pytest.mark.parametrize("w", [0.0, 0.3])
def test_a_peaked_lm_forces_its_chain_through_the_joint_search(gpu, w):
    from onebit_asr.attdec import joint_beam_search

    model, _ = tj._decoder_model(35, 64)
    enc, mask = tj._memory(0, 64, (61, 20, 7), gpu)
    with torch.no_grad():
        z = model.ctc_logits(enc)
    lm = _chain_lm(35)
    hyp, hyp_len, n_hyp, _, info = joint_beam_search(model, enc, mask, z, 4, 10, w, 32, lm=lm,
                                                     lm_weight=50.0)
    hyp0, len0, _, _, _ = joint_beam_search(model, enc, mask, z, 4, 10, w, 32)
    for b in range(3):
        assert hyp[b, 0, :hyp_len[b, 0]].tolist() == CHAIN and bool(info["finished"][b, 0])
        assert hyp0[b, 0, :len0[b, 0]].tolist() != CHAIN


def test_a_peaked_lm_forces_its_chain_through_the_rescored_beam(gpu):
    from onebit_asr.infer import ctc_beam_search_nbest_device, ctc_lm_rescore

    model, _ = tj._decoder_model(35, 64)
    enc, mask = tj._memory(0, 64, (61, 20, 7), gpu)
    with torch.no_grad():
        z = model.ctc_logits(enc).float()
    lens = mask.sum(1)
    hyp, hyp_len, n_hyp, sc = ctc_beam_search_nbest_device(z, lens, 4, None, BLANK, None)
    h_, l_, n_, s_ = (t.cpu().numpy().copy() for t in (hyp, hyp_len, n_hyp, sc))
    for b in range(3):
        assert h_[b, 0, :l_[b, 0]].tolist() != CHAIN            # without the LM: not the chain
        if not any(h_[b, k, :l_[b, k]].tolist() == CHAIN for k in range(n_[b])):
            k = min(n_[b], 3)                                   # insert it, as the worst entry
            h_[b, k] = -1
            h_[b, k, :len(CHAIN)] = CHAIN
            l_[b, k] = len(CHAIN)
            s_[b, k] = s_[b, :max(n_[b], 1)].min() - 5.0
            n_[b] = k + 1
    args = [torch.from_numpy(a).to(gpu) for a in (h_, l_, n_, s_)]
    out, cnt, info = ctc_lm_rescore(*args, _chain_lm(35), 50.0, 35)
    for b in range(3):
        assert out[b, :cnt[b]].tolist() == CHAIN and (out[b, cnt[b]:] == -1).all()
        k = int(info["best_k"][b])
        assert h_[b, k, :l_[b, k]].tolist() == CHAIN


# ------------------------------------------------------------------------------------------
# 6. the LM pick and the no-op guarantees
# ------------------------------------------------------------------------------------------
def test_rescore_select_lm_equals_the_float64_formula(gpu):
    from onebit_asr.infer import attention_rescore, ctc_beam_search_nbest_device, ctc_lm_rescore

    model, _ = tj._decoder_model(35, 64)
    enc, mask = tj._memory(0, 64, tj.LENS, gpu)
    lm, ref_lm = _lm(3, 35)
    with torch.no_grad():
        z = model.ctc_logits(enc).float()
    nbest = ctc_beam_search_nbest_device(z, mask.sum(1), 6, None, BLANK, None)
    hyp, hyp_len, n_hyp, sc = nbest
    base = attention_rescore(model, enc, mask, *nbest, 0.4, 61)
    out, cnt, info = attention_rescore(model, enc, mask, *nbest, 0.4, 61, lm=lm, lm_weight=0.7)
    assert _bytes(info["att"]) == _bytes(base[2]["att"])
    att, lms, ctc = (t.cpu().numpy() for t in (info["att"], info["lm"], sc))
    n_ = n_hyp.cpu().numpy()
    for b in range(3):
        for k in range(6):
            toks = hyp[b, k, :hyp_len[b, k]].tolist()
            assert lms[b, k] == (ref_lm.seq_logprob(toks) if k < n_[b] else NEG_INF)
    with np.errstate(invalid="ignore"):
        want = (att + 0.4 * ctc) + 0.7 * lms
    live = np.arange(6)[None, :] < n_[:, None]
    want = np.where(live, want, NEG_INF)
    assert info["total"].cpu().numpy().tobytes() == want.tobytes()
    assert info["best_k"].cpu().tolist() == [int(np.argmax(want[b])) for b in range(3)]
    assert bool(info["rescored"].all())
    for b in range(3):
        k = int(info["best_k"][b])
        assert out[b, :cnt[b]].tolist() == hyp[b, k, :hyp_len[b, k]].tolist()
    # the form without an attention pass
    out2, cnt2, info2 = ctc_lm_rescore(*nbest, lm, 0.7, 35)
    want2 = np.where(live, ctc + 0.7 * lms, NEG_INF)
    assert info2["total"].cpu().numpy().tobytes() == want2.tobytes()
    assert info2["best_k"].cpu().tolist() == [int(np.argmax(want2[b])) for b in range(3)]
    # a tie goes to the smaller k: two equal entries with equal CTC scores, and an absent third
    h = torch.tensor([[[5, 6, -1], [7, -1, -1], [7, -1, -1], [9, 9, 9]]], dtype=torch.int32,
                     device=gpu)
    ln = torch.tensor([[2, 1, 1, 3]], dtype=torch.int32, device=gpu)
    c = torch.tensor([[-9.0, -1.0, -1.0, 0.0]], dtype=torch.float64, device=gpu)
    o3, c3, i3 = ctc_lm_rescore(h, ln, torch.tensor([3], dtype=torch.int32, device=gpu), c, lm,
                                0.25, 35)
    tot = i3["total"][0].cpu().tolist()
    assert tot[1] == tot[2] == -1.0 + 0.25 * ref_lm.seq_logprob([7]) and tot[3] == NEG_INF
    assert tot[0] == -9.0 + 0.25 * ref_lm.seq_logprob([5, 6])
    assert int(i3["best_k"][0]) == (1 if tot[1] >= tot[0] else 0)
    assert o3[0, :c3[0]].tolist() == ([7] if tot[1] >= tot[0] else [5, 6])


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, dict):
            assert x.keys() == y.keys(), (sorted(x), sorted(y))
            for k in x:
                assert x[k].dtype == y[k].dtype and _bytes(x[k]) == _bytes(y[k]), k
        else:
            assert x.dtype == y.dtype and _bytes(x) == _bytes(y)


@pytest.mark.parametrize("w", [0.0, 0.3])
def test_no_lm_is_bitwise_the_search_and_the_rescoring_of_today(gpu, w):
    from onebit_asr.attdec import joint_beam_search
    from onebit_asr.infer import attention_rescore, ctc_beam_search_nbest_device
    from onebit_asr.metrics import (ctc_attention_rescore_batch, ctc_lm_rescore_batch,
                                    joint_decode_batch)

    model, _ = tj._decoder_model(35, 64)
    enc, mask = tj._memory(0, 64, tj.LENS + (0,), gpu)
    lm, _ = _lm(3, 35)
    with torch.no_grad():
        z = model.ctc_logits(enc).float()
    ref = joint_beam_search(model, enc, mask, z, 4, 8, w, None, 0.6)
    _same(ref, joint_beam_search(model, enc, mask, z, 4, 8, w, None, 0.6, lm=lm, lm_weight=0.0))
    _same(ref, joint_beam_search(model, enc, mask, z, 4, 8, w, None, 0.6, lm=None, lm_weight=0.7))
    assert "lm" not in ref[4]
    fused = joint_beam_search(model, enc, mask, z, 4, 8, w, None, 0.6, lm=lm, lm_weight=0.7)
    assert "lm" in fused[4] and _bytes(fused[3]) != _bytes(ref[3])
    enc, mask, z = enc[:3], mask[:3], z[:3].contiguous()   # (the rescoring: no empty utterance)
    lens = mask.sum(1)
    nbest = ctc_beam_search_nbest_device(z, lens, 4, None, BLANK, None)
    ref2 = attention_rescore(model, enc, mask, *nbest, 0.5 + w, 61)
    _same(ref2, attention_rescore(model, enc, mask, *nbest, 0.5 + w, 61, lm=lm, lm_weight=0.0))
    _same(ref2, attention_rescore(model, enc, mask, *nbest, 0.5 + w, 61, lm=None, lm_weight=0.7))
    assert "lm" not in ref2[2]
    # the metrics wrappers
    assert joint_decode_batch(model, enc, mask, z, 4, 8, w, lm=lm, lm_weight=0.0) == \
        joint_decode_batch(model, enc, mask, z, 4, 8, w)
    f_hyp, f_len = joint_beam_search(model, enc, mask, z, 4, 8, w, lm=lm, lm_weight=0.7)[:2]
    assert joint_decode_batch(model, enc, mask, z, 4, 8, w, lm=lm, lm_weight=0.7) == \
        [f_hyp[b, 0, :f_len[b, 0]].tolist() for b in range(3)]
    assert ctc_attention_rescore_batch(model, enc, mask, z, lens, 4, BLANK, 0.5, 61, lm=lm) == \
        ctc_attention_rescore_batch(model, enc, mask, z, lens, 4, BLANK, 0.5, 61)
    assert len(ctc_lm_rescore_batch(z, lens, lm, 0.7, 4)) == 3


@functools.lru_cache(maxsize=None)
def _full_model():
    from onebit_asr.conformer import ConformerASR
    from onebit_asr.data import CFG1, synthetic_batch

    torch.manual_seed(0)
    model = ConformerASR(80, 5004, **CFG1).to("cuda:0").eval()
    feat_lens, tok_lens = [349, 61], [12, 3]
    return model, [synthetic_batch(feat_lens, tok_lens, seed=s, device="cuda:0") for s in (0, 1)]


DECODERS = [("greedy", {}), ("beam", {}), ("rescore", dict(max_len=24)),
            ("attention", dict(max_len=12)), ("attention", dict(max_len=12, joint_ctc_weight=0.3))]


@pytest.mark.parametrize("decoder,kw", DECODERS, ids=[d + ("-joint" if "joint_ctc_weight" in k
                                                           else "") for d, k in DECODERS])
def test_encode_and_decode_without_lm_weight_is_bitwise_unchanged(gpu, decoder, kw):
    from onebit_asr.infer import encode_and_decode
    from onebit_asr.quant import set_act_quant

    model, batches = _full_model()
    set_act_quant(model, None)
    lm, _ = _lm(4, 5004)
    runs = []
    for extra in ({}, dict(lm=lm, lm_weight=0.0), dict(lm=None, lm_weight=0.0)):
        info = {}
        out, cnt, logits = encode_and_decode(model, batches[0], decoder=decoder, beam_size=4,
                                             info=info, **kw, **extra)
        runs.append((out, cnt, logits, info))
    _same(runs[0], runs[1])
    _same(runs[0], runs[2])
    if decoder == "greedy":
        with pytest.raises(ValueError, match="greedy"):
            encode_and_decode(model, batches[0], decoder="greedy", lm=lm, lm_weight=0.5)
        return
    info = {}
    out, cnt, _ = encode_and_decode(model, batches[0], decoder=decoder, beam_size=4, info=info,
                                    lm=lm, lm_weight=0.5, **kw)
    assert "lm" in info and info["lm"].dtype == torch.float64
    if decoder == "beam":
        assert set(info) >= {"hyp", "hyp_len", "n_hyp", "ctc_scores", "lm", "total", "best_k"}
        for b in range(2):
            k = int(info["best_k"][b])
            assert out[b, :cnt[b]].tolist() == info["hyp"][b, k, :info["hyp_len"][b, k]].tolist()


# ------------------------------------------------------------------------------------------
# 7. graphed
# ------------------------------------------------------------------------------------------
GRAPHED = [("beam", {}, ("hyp", "hyp_len", "n_hyp", "ctc_scores", "lm", "total", "best_k")),
           ("rescore", dict(max_len=24), ("best_k", "att", "total", "lm", "rescored")),
           ("attention", dict(max_len=12, joint_ctc_weight=0.3),
            ("hyp", "hyp_len", "n_hyp", "score", "finished", "trace_parent", "trace_token",
             "trace_score", "att", "ctc", "lm"))]


@pytest.mark.parametrize("decoder,kw,keys", GRAPHED, ids=[g[0] for g in GRAPHED])
def test_graphed_decoding_with_an_lm_equals_eager_bitwise(gpu, decoder, kw, keys):
    from onebit_asr.infer import GraphedInference, encode_and_decode
    from onebit_asr.quant import set_act_quant

    model, (b1, b2) = _full_model()
    lm, _ = _lm(4, 5004)
    gi = GraphedInference(model, act_quant=None, decoder=decoder, beam_size=4, lm=lm,
                          lm_weight=0.5, **kw)
    runs = []
    for b in (b1, b1, b2, b1):
        out, cnt, _ = gi.run(b)
        runs.append((out.clone(), cnt.clone(), {k: gi.info[k].clone() for k in keys}))
    assert gi.graph is not None
    set_act_quant(model, None)
    eager = []
    for b in (b1, b2):
        info = {}
        ekw = dict(kw)
        out, cnt, _ = encode_and_decode(model, b, decoder=decoder, beam_size=4, info=info, lm=lm,
                                        lm_weight=0.5, **ekw)
        eager.append((out, cnt, {k: info[k] for k in keys}))
    _same(runs[0], eager[0])
    _same(runs[1], runs[0])
    _same(runs[3], runs[0])
    _same(runs[2], eager[1])


# ------------------------------------------------------------------------------------------
# 8. the one loop's phases, driven by hand (what tools/joint_bench.py and ngram_bench.py rest on)
# ------------------------------------------------------------------------------------------
def _tensors(x):
    """The tensors of a state, in a fixed order."""
    if isinstance(x, torch.Tensor):
        return [x]
    if isinstance(x, dict):
        return [t for k in sorted(x) for t in _tensors(x[k])]
    if isinstance(x, (list, tuple)):
        return [t for v in x for t in _tensors(v)]
    return []


def _raw(x):
    return [t.contiguous().view(torch.uint8).cpu().numpy().tobytes() for t in _tensors(x)]


#           joint  w    LM     entry                    CTC scorer  LM scorer
PHASES = [(False, 0.0, False, "ob_attdec_beam_step", False, False),
          (True, 0.3, False, "ob_attdec_joint_step", True, False),
          (True, 0.0, False, "ob_attdec_beam_step", False, False),
          (True, 0.0, True, "ob_attdec_fused_step", False, True),
          (True, 0.3, True, "ob_attdec_fused_step", True, True)]


@pytest.mark.parametrize("joint,w,with_lm,entry,ctc,lms", PHASES,
                         ids=["attention", "joint", "joint-w0", "fused-w0", "fused"])
def test_the_phases_by_hand_are_bitwise_the_public_search(gpu, golden_dir, joint, w, with_lm,
                                                          entry, ctc, lms):
    """V = 35, d = 64, B = 4 (one empty-mask utterance), N = 4, K = 8, L = 8, length penalty 0.6,
    the tiny golden LM: propose / score_ctc / score_lm / select for every t and finish() give all
    five items of the public function bytewise, and a select on a cloned state at t = 3 changes
    neither the search's own state nor its result."""
    from onebit_asr.attdec import SPECIAL, _BeamSearch, attention_beam_search, joint_beam_search
    from onebit_asr.ngram import NGramLM

    model, _ = tj._decoder_model(35, 64)
    enc, mask = tj._memory(0, 64, tj.LENS + (0,), gpu)
    N, K, L, alpha, lw = 4, 8, 8, 0.6, 0.7
    lm = NGramLM.from_arpa(golden_dir / "ngram_tiny.arpa") if with_lm else None
    with torch.no_grad():
        z = model.ctc_logits(enc).float().contiguous()
    if joint:
        want = joint_beam_search(model, enc, mask, z, N, L, w, K, alpha, lm=lm, lm_weight=lw)
        bs = _BeamSearch(model, enc, mask, N, K, L, alpha, SPECIAL, z, w, lm, lw)
    else:
        want = attention_beam_search(model, enc, mask, N, L, alpha)
        bs = _BeamSearch(model, enc, mask, N, None, L, alpha, SPECIAL)
    assert (bs.mode.entry, bs.mode.k, bs.mode.ctc, bs.mode.lm) == (entry, K if joint else N, ctc,
                                                                   lms)
    assert set(want[4]) == {"finished", "trace_parent", "trace_token", "trace_score"} | \
        ({"att", "ctc"} if joint else set()) | ({"lm"} if with_lm else set())
    # a mode allocates only what it uses
    assert ("att" in bs.state, "link" in bs.state) == (joint, joint)
    assert ("cpsi" in bs.state, "ctc_state" in bs.state) == (ctc, ctc)
    assert ("lm" in bs.state, "lmctx" in bs.state, "lmsc" in bs.state) == (lms, lms, lms)
    for t in range(L):
        bs.propose(t)
        if ctc:
            bs.score_ctc(t)
        if lms:
            bs.score_lm(t)
        if t == 3:
            before = _raw(bs.state)
            clone = bs.clone_state()
            assert _raw(clone) == before
            bs.select(t, clone)
            assert _raw(bs.state) == before           # the search's own state: untouched
            assert _bytes(clone["length"]) != _bytes(bs.state["length"])   # the clone's: advanced
        bs.select(t)
        if t == 3:
            assert _raw(clone) == _raw(bs.state)      # the same step from the same state
    _same(want, bs.finish())
