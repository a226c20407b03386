"""GPU: the joint CTC/attention beam search (csrc/ctcprefix.hip, the joint step of
csrc/attdec.hip, ``onebit_asr.attdec.joint_beam_search``) against the float64 oracle of
tests/joint_ref.py.

Bars.
* Frame log-sum-exp: 1e-9 against float64; frames past ``lens`` keep a poison value.
* Scorer step: ``cpsi`` and the stored states within 1e-9 * max(1, T) of the oracle (the project's
  bar for fp64 CTC scores from fp32 logits), -inf exactly; the same bits under a permuted slot
  assignment; skipped rows and frames past T untouched.
* Joint beam step / finalize: equal to the oracle bookkeeping exactly (binary fractions).
* End to end: the step-wise rule of ``joint_ref.check_joint_search`` with e = 4x the error of the
  existing attention path (``model.decode_logits`` on the GPU, log-softmax in float64 on the
  host) + 1e-9 * max(1, T); where the oracle's smallest margin is >= 10e the n-best, finished, S,
  A and C equal the oracle's. Every N = 1 case and the T = 1 utterance of every V = 35 case must
  be decisive.
* Weight 0: bitwise equal to ``attention_beam_search``. Graphed: bitwise equal to eager, replays
  bitwise equal.

Figures seen on an MI355X (each test prints its own, -s; log profiles/r9/joint_gpu_tests.log):
frame lse error at most 1.8e-15; scorer ``cpsi`` error at most 7.1e-15 and state error at most
1.4e-14 (T' = 256, V = 5004), 1068 -inf entries exact; end to end e is 8.2e-7 to 7.7e-6 and the
device S error at most 1.5e-6. Oracle margins at V = 35: N = 1 at least 1.2e-2, the T = 1
utterance at least 7.2e-3, the rest 5.5e-5 (N = 10, w = 0.5, T = 61) to 2.1e-2, all decisive and
equal to the oracle's n-best; the T = 1 utterance drops 31 / 124 / 279-310 candidates (N = 1 / 4 /
10) and finishes every slot. Shifted biases: 0, 9 and 10 of 10 slots finished at T = 61, 20, 1.
V = 5004, K = 20: margins 8.2e-5, 2.3e-5 (not decisive), the T = 1 utterance ends with
``n_hyp`` 0 after 200 drops.
"""
import copy
import functools
import math

import numpy as np
import pytest
import torch

import attdec_ref as ar
import joint_ref as jr
import rescore_ref as rr

pytestmark = pytest.mark.gpu

NEG_INF = -math.inf
PAD, BOS, EOS, BLANK = 0, 1, 2, 3


def _bytes(t):
    return t.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------
# 1. frame log-sum-exp
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Tp,V,lens", [(1, 1, 5, (1,)), (3, 7, 64, (7, 0, 3)),
                                         (2, 61, 5004, (61, 20))])
def test_frame_lse_matches_float64(gpu, B, Tp, V, lens):
    from onebit_asr.attdec import ctc_frame_lse

    rng = np.random.default_rng(9000 + V)
    z = (rng.standard_normal((B, Tp, V)) * 3.0).astype(np.float32)
    z[0, 0, V - 1] = 40.0   # one dominant logit
    z64 = z.astype(np.float64)
    m = z64.max(-1, keepdims=True)
    ref = (m + np.log(np.exp(z64 - m).sum(-1, keepdims=True)))[..., 0]
    out = torch.full((B, Tp), 77.0, dtype=torch.float64, device=gpu)
    got = ctc_frame_lse(torch.from_numpy(z).to(gpu), torch.tensor(lens), out).cpu().numpy()
    worst = 0.0
    for b, n in enumerate(lens):
        assert (got[b, n:] == 77.0).all()
        if n:
            worst = max(worst, float(np.abs(got[b, :n] - ref[b, :n]).max()))
    print(f"B={B} T'={Tp} V={V}: frame lse err {worst:.3e}")
    assert worst <= 1e-9
    again = ctc_frame_lse(torch.from_numpy(z).to(gpu), torch.tensor(lens),
                          torch.full((B, Tp), 77.0, dtype=torch.float64, device=gpu))
    assert _bytes(again) == got.tobytes()


# ------------------------------------------------------------------------------------------
# 2. the scorer step alone, along oracle-chosen prefixes
# ------------------------------------------------------------------------------------------
#                B  N   K   T'   V     lens
SCORER_CASES = [(1, 1, 1, 1, 5, (1,)), (2, 3, 5, 7, 9, (7, 7)), (3, 10, 32, 61, 35, (61, 20, 1)),
                (2, 4, 8, 256, 5004, (256, 130))]
SCORER_STEPS = 4


@functools.lru_cache(maxsize=None)
def _scorer_plan(i):
    """The logical tree of a case: per step and utterance N nodes (parent node, token appended,
    the K candidates to score, skipped), its float64 oracle, and what the case covers."""
    B, N, K, Tp, V, lens = SCORER_CASES[i]
    rng = np.random.default_rng(9100 + i)
    z = (rng.standard_normal((B, Tp, V)) * 2.0).astype(np.float32)
    x = [jr.log_softmax64(z[b, :lens[b]]) for b in range(B)]
    usable = [v for v in range(V) if v not in (PAD, BOS, BLANK, EOS)]
    cover = set()
    steps = []
    prev = None
    for s in range(SCORER_STEPS):
        nodes = []
        for b in range(B):
            for j in range(N):
                if s == 0:
                    par, tok, toks = -1, -1, []
                    gn, gb = jr.root(x[b], BLANK)
                    cover.add("empty")
                else:
                    choices = [q for q in range(N) if not prev[b * N + q]["skip"]]
                    par = int(rng.choice(choices))
                    pn = prev[b * N + par]
                    real = [int(c) for c in pn["cand"] if c >= 0 and c != EOS]
                    tok = int(rng.choice(real))
                    toks = pn["toks"] + [tok]
                    gn, gb, _ = jr.extend(x[b], BLANK, pn["toks"], pn["gn"], pn["gb"], tok)
                cand = [int(c) for c in rng.choice(usable, size=min(K, len(usable)),
                                                   replace=False)]
                cand += [-1] * (K - len(cand))
                if toks and K >= 1 and (j % 2 == 0 or K == 1):
                    cand[0] = toks[-1]                       # a candidate equal to the last token
                    cover.add("repeat")
                if K >= 2 and j % 3 != 2:
                    cand[1] = EOS
                    cover.add("eos")
                if K >= 3:
                    cand[K - 1] = -1
                    cover.add("pad")
                skip = N > 1 and s == 2 and b == B - 1 and j == N - 1
                if skip:
                    cover.add("skip")
                want = []
                for c in cand:
                    if c < 0:
                        want.append(NEG_INF)
                    elif c == EOS:
                        want.append(jr.eos_score(gn, gb))
                    else:
                        want.append(jr.extend(x[b], BLANK, toks, gn, gb, c)[2])
                        if want[-1] == NEG_INF:
                            cover.add("impossible")
                nodes.append(dict(par=par, tok=tok, toks=toks, gn=gn, gb=gb, cand=cand,
                                  skip=skip, want=want))
        steps.append(nodes)
        prev = nodes
    return z, steps, cover


def _drive_scorer(gpu, i, seed):
    """Run the plan with a random slot placement per step (seed None: the identity); returns per
    step (cpsi [R, K], state [R, T', 2]) in LOGICAL node order."""
    from onebit_asr.attdec import ctc_frame_lse, ctc_prefix_step

    B, N, K, Tp, V, lens = SCORER_CASES[i]
    R = B * N
    z, steps, _ = _scorer_plan(i)
    rng = np.random.default_rng(seed) if seed is not None else None
    dz = torch.from_numpy(z).to(gpu)
    dlens = torch.tensor(lens, dtype=torch.int64, device=gpu)
    flse = ctc_frame_lse(dz, dlens, torch.full((B, Tp), float("nan"), dtype=torch.float64,
                                               device=gpu))
    state = torch.full((2, R, Tp, 2), float("nan"), dtype=torch.float64, device=gpu)
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
        link = np.full((R, 2), -7, np.int32)      # (rubbish where it must not be read)
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
        cpsi = torch.full((R, K), 77.0, dtype=torch.float64, device=gpu)
        st_out = state[(s + 1) & 1]
        st_out.fill_(77.0)
        ctc_prefix_step(dz, flse, dlens, torch.from_numpy(topi).to(gpu),
                        torch.from_numpy(tok).to(gpu), torch.from_numpy(length).to(gpu),
                        torch.from_numpy(link).to(gpu), torch.from_numpy(skip).to(gpu),
                        state[s & 1], st_out, cpsi, BLANK, EOS)
        idx = torch.from_numpy(place).to(gpu)
        out.append((cpsi[idx].cpu().numpy(), st_out[idx].cpu().numpy()))
        place_prev = place
    return out


@pytest.mark.parametrize("i", range(len(SCORER_CASES)),
                         ids=["x".join(map(str, c[:5])) for c in SCORER_CASES])
def test_scorer_step_matches_the_oracle_and_follows_the_parent(gpu, i):
    B, N, K, Tp, V, lens = SCORER_CASES[i]
    _, steps, cover = _scorer_plan(i)
    runs = [_drive_scorer(gpu, i, seed) for seed in (None, 1, 2)]
    worst_c = worst_s = 0.0
    n_inf = 0
    for s, nodes in enumerate(steps):
        cpsi, st = runs[0][s]
        for other in runs[1:]:                         # the same bits wherever the prefix sits
            assert other[s][0].tobytes() == cpsi.tobytes(), s
            assert other[s][1].tobytes() == st.tobytes(), s
        assert not np.isnan(cpsi).any() and not np.isnan(st).any()
        for q, nd in enumerate(nodes):
            T = lens[q // N]
            tol = 1e-9 * max(1, T)
            assert (st[q, T:] == 77.0).all()           # frames past T: untouched
            if nd["skip"]:
                assert (cpsi[q] == 77.0).all() and (st[q] == 77.0).all()
                continue
            for got, want in zip(cpsi[q], nd["want"]):
                if want == NEG_INF:
                    n_inf += 1
                    assert got == NEG_INF, (s, q, got)
                else:
                    worst_c = max(worst_c, abs(got - want))
                    assert abs(got - want) <= tol, (s, q, got, want)
            for t in range(T):
                for got, want in ((st[q, t, 0], nd["gb"][t]),
                                  (st[q, t, 1], jr.lse(nd["gn"][t], nd["gb"][t]))):
                    if want == NEG_INF:
                        assert got == NEG_INF, (s, q, t)
                    else:
                        worst_s = max(worst_s, abs(got - want))
                        assert abs(got - want) <= tol, (s, q, t, got, want)
    print(f"B={B} N={N} K={K} T'={Tp} V={V}: cpsi err {worst_c:.3e} state err {worst_s:.3e} "
          f"({n_inf} -inf exact) covers {sorted(cover)}")


def test_scorer_cases_cover_what_they_claim():
    cover = set()
    for i in range(len(SCORER_CASES)):
        cover |= _scorer_plan(i)[2]
    assert cover >= {"empty", "repeat", "eos", "pad", "impossible", "skip"}, cover


# ------------------------------------------------------------------------------------------
# 3. the joint beam step / finalize against the oracle bookkeeping
# ------------------------------------------------------------------------------------------
def _hash_cscore(seed):
    """C' of (prefix, token): a multiple of 1/64 in [-8, 0], -inf for one candidate in five."""
    import zlib

    def cscore(toks, v):
        h = zlib.crc32(repr((seed, tuple(toks), int(v))).encode())
        return NEG_INF if h % 5 == 0 else -float((h >> 8) % 513) / 64.0
    return cscore


def _run_joint_bookkeeping(gpu, logps, cscores, alive, N, K, L, w, alpha, V):
    from onebit_asr import _lib
    from onebit_asr.attdec import length_norm

    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    banned = {PAD, BOS, BLANK}
    B = len(logps)
    R = B * N
    x0 = np.zeros((1, V))
    refs = [jr.joint_search(lp, x0, N, K, L, w, alpha, alive=a, cscore=cs)
            for lp, cs, a in zip(logps, cscores, alive)]
    kmask = torch.zeros(B, 3, dtype=torch.uint8, device=gpu)
    for b, a in enumerate(alive):
        if not a:
            kmask[b] = 1
    f64 = torch.float64
    score = torch.full((B, N), 5.0, dtype=f64, device=gpu)
    att = torch.zeros((B, N), dtype=f64, device=gpu)
    ctc = torch.zeros((B, N), dtype=f64, device=gpu)
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
        for b in range(B):
            slots = refs[b].history[t]
            live = [k for k, s in enumerate(slots) if s is not None and not s.fin]
            assert skip.cpu().tolist()[b * N:(b + 1) * N] == [0 if k in live else 1
                                                              for k in range(N)]
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
        d_lse, d_v, d_i, d_c = (torch.from_numpy(a).to(gpu) for a in (lse, topv, topi, cpsi))
        assert lib.ob_attdec_joint_step(
            d_lse.data_ptr(), d_v.data_ptr(), d_i.data_ptr(), d_c.data_ptr(), w, B, N, K, L, t, EOS,
            PAD, norm.data_ptr(), anc[t & 1].data_ptr(), anc[(t + 1) & 1].data_ptr(),
            score.data_ptr(), att.data_ptr(), ctc.data_ptr(), length.data_ptr(), fin.data_ptr(),
            tok.data_ptr(), skip.data_ptr(), link.data_ptr(), trp.data_ptr(), trt.data_ptr(),
            trs.data_ptr(), st) == 0
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
@pytest.mark.parametrize("w", [0.25, 0.5])
@pytest.mark.parametrize("N,K", [(1, 1), (1, 2), (4, 4), (4, 8), (10, 10), (10, 20)])
def test_joint_step_and_finalize_match_the_oracle(gpu, N, K, w, alpha):
    V, L = 40, 6
    logps = [jr.hash_logp(100 * N + u, V, EOS) for u in range(4)]
    cs = [_hash_cscore(7 * N + u) for u in range(4)]
    refs = _run_joint_bookkeeping(gpu, logps, cs, [True, True, False, True], N, K, L, w, alpha, V)
    assert refs[2].hyps == []
    assert sum(r.dropped for r in refs) > 0          # some candidates were CTC-impossible


# ------------------------------------------------------------------------------------------
# 4.-6. end to end, eager, on synthetic memory
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
    """test_attdec_gpu.py's synthetic encoder output."""
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(len(LENS), 61, d, generator=g)
    mask = torch.zeros(len(lens), 61, dtype=torch.long)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    if len(lens) > len(LENS):
        enc = torch.cat([enc, torch.randn(len(lens) - len(LENS), 61, d, generator=g)])
    return enc.to(gpu), mask.to(gpu)


def _existing_logp(model, enc_b, mask_b, bos=BOS):
    def logp(prefixes):
        n = len(prefixes)
        inp = torch.tensor([[bos] + list(p) for p in prefixes], dtype=torch.long,
                           device=enc_b.device)
        with torch.no_grad():
            z = model.decode_logits(enc_b[None].repeat(n, 1, 1), mask_b[None].repeat(n, 1), inp,
                                    torch.zeros(inp.shape, dtype=torch.bool, device=enc_b.device))
        return torch.log_softmax(z[:, -1].double().cpu(), dim=-1).numpy()
    return logp


def _memo(fn):
    """A ``logp`` that computes every prefix once (the oracle search and the step-wise check
    visit the same prefixes)."""
    seen = {}

    def logp(prefixes):
        miss = [p for p in prefixes if tuple(p) not in seen]
        if miss:
            for p, lp in zip(miss, fn(miss)):
                seen[tuple(p)] = lp
        return [seen[tuple(p)] for p in prefixes]
    return logp


def _check_joint(gpu, model, model64, enc, mask, N, L, K, w, tag, decisive_utts=(), exact=True,
                 alpha=0.0):
    from onebit_asr.attdec import joint_beam_search

    B = enc.shape[0]
    with torch.no_grad():
        z = model.ctc_logits(enc).float().contiguous()
    hyp, hyp_len, n_hyp, score, info = joint_beam_search(model, enc, mask, z, N, L, w, K, alpha)
    K = min(32, 2 * N) if K is None else K      # the default pre-beam
    assert hyp.shape == (B, N, L) and score.dtype == torch.float64
    assert info["att"].shape == info["ctc"].shape == (B, N) and info["att"].dtype == torch.float64
    h_, l_, n_, s_ = (t.cpu().numpy() for t in (hyp, hyp_len, n_hyp, score))
    a_, c_, f_ = (info[k].cpu().numpy() for k in ("att", "ctc", "finished"))
    tp, tt, ts = (info[k].cpu().numpy() for k in ("trace_parent", "trace_token", "trace_score"))
    assert not np.isnan(s_).any() and not np.isnan(a_).any() and not np.isnan(c_).any()
    assert not np.isnan(ts).any()
    enc64, mask_c, z_c = enc.cpu().numpy(), mask.cpu().numpy(), z.cpu().numpy()
    results = []
    for b in range(B):
        T = int(mask_c[b].sum())
        got = [h_[b, k, :l_[b, k]].tolist() for k in range(n_[b])]
        fins = [bool(f_[b, k]) for k in range(n_[b])]
        for k in range(N):
            assert (h_[b, k, l_[b, k]:] == -1).all()
            if k >= n_[b]:
                assert l_[b, k] == 0 and s_[b, k] == a_[b, k] == c_[b, k] == NEG_INF
                assert not f_[b, k]
        if T == 0:
            assert n_[b] == 0 and (tt[:, b] == ar.DEAD).all() and (ts[:, b] == NEG_INF).all()
            results.append((got, fins, None))
            continue
        x = jr.log_softmax64(z_c[b, :T])
        logp64 = _memo(ar.model_logp(model64, enc64[b], mask_c[b]))
        e, worst, final, last, dropped = jr.check_joint_search(
            tp[:, b], tt[:, b], ts[:, b], logp64, _existing_logp(model, enc[b], mask[b]), x, N, K,
            L, w, alpha)
        live = [(s, fc) for s, fc in zip(last, final) if s is not None]
        assert got == [s.toks for s, _ in live] and fins == [s.fin for s, _ in live]
        assert s_[b, :n_[b]].tolist() == [s.score for s, _ in live]
        for k, (s, (oa, oc)) in enumerate(live):     # the returned A / C along the device's path
            assert abs(a_[b, k] - oa) <= e and abs(c_[b, k] - oc) <= e, (b, k)
            assert s_[b, k] == (1.0 - w) * a_[b, k] + w * c_[b, k]
        ref = jr.joint_search(logp64, x, N, K, L, w, alpha)
        decisive = ref.margin >= 10 * e
        print(f"{tag} utt {b} (T={T}): e {e:.3e} device S err {worst:.3e} oracle margin "
              f"{ref.margin:.3e} decisive {decisive} finished {sum(fins)}/{n_[b]} "
              f"dropped {dropped} (oracle search {ref.dropped})")
        if b in decisive_utts:
            assert decisive, (b, ref.margin, e)
        if decisive and exact:
            assert got == ref.hyps and fins == ref.finished, (b, got, ref.hyps)
            for k in range(n_[b]):
                assert abs(s_[b, k] - ref.scores[k]) <= e
                assert abs(a_[b, k] - ref.att[k]) <= e and abs(c_[b, k] - ref.ctc[k]) <= e
        results.append((got, fins, ref))
    return results


E2E = [(N, L, w) for N, L in ((1, 12), (4, 8), (10, 12)) for w in (0.3, 0.5)]


@pytest.mark.parametrize("N,L,w", E2E, ids=[f"N{N}-L{L}-w{w}" for N, L, w in E2E])
def test_joint_search_end_to_end_v35(gpu, N, L, w):
    """V = 35: 32 unbanned ids, so K = 32 takes the pre-beam out of the comparison."""
    model, model64 = _decoder_model(35, 64)
    enc, mask = _memory(0, 64, LENS, gpu)
    res = _check_joint(gpu, model, model64, enc, mask, N, L, 32, w, f"V=35 N={N} L={L} w={w}",
                       decisive_utts=(0, 1, 2) if N == 1 else (2,))
    got, fins, ref = res[2]                 # T = 1: one token at most, then only eos aligns
    assert all(fins) and len(fins) >= 1 and all(len(h) <= 1 for h in got)
    assert ref.dropped >= 31                # every second token of a live slot is impossible


def test_joint_search_finishes_through_the_ctc_term(gpu):
    base, _ = _decoder_model(35, 64)
    model = copy.deepcopy(base)
    with torch.no_grad():
        model.decoder.out.bias[EOS] += 0.75
        model.ctc_head.bias[BLANK] += 3.0
    model64 = rr.double_model(model)
    enc, mask = _memory(0, 64, LENS, gpu)
    res = _check_joint(gpu, model, model64, enc, mask, 10, 12, 32, 0.3, "ctc-finish")
    refs = [r for _, _, r in res]
    print("oracle finished per utterance:", [sum(r.finished) for r in refs],
          "of", [len(r.finished) for r in refs])
    assert any(any(r.finished) and not all(r.finished) for r in refs)   # both kinds in one beam
    assert any(r.finished and not any(r.finished) for r in refs)        # and a beam with none


def test_joint_search_pre_beam_v5004(gpu):
    model, model64 = _decoder_model(5004, 64)
    enc, mask = _memory(0, 64, LENS, gpu)
    res = _check_joint(gpu, model, model64, enc, mask, 10, 12, 20, 0.3, "V=5004 K=20", exact=False)
    got, fins, ref = res[2]
    assert ref.hyps == [] and got == []     # T = 1, eos outside every row's 20 candidates


def test_joint_search_d144_and_all_masked(gpu):
    model, model64 = _decoder_model(35, 144)        # d = 144, H = 4: dh = 36
    enc, mask = _memory(0, 144, LENS + (0,), gpu)
    res = _check_joint(gpu, model, model64, enc, mask, 4, 8, None, 0.3, "d=144 K=8", alpha=0.6)
    assert res[3] == ([], [], None)


# ------------------------------------------------------------------------------------------
# 7. weight 0
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,alpha", [(1, 6, 0.0), (4, 8, 0.6)])
def test_weight_zero_equals_the_attention_search_bitwise(gpu, N, L, alpha):
    from onebit_asr.attdec import attention_beam_search, joint_beam_search

    model, _ = _decoder_model(35, 64)
    enc, mask = _memory(0, 64, LENS + (0,), gpu)
    with torch.no_grad():
        z = model.ctc_logits(enc)
    ref = attention_beam_search(model, enc, mask, N, L, alpha)
    got = joint_beam_search(model, enc, mask, z, N, L, 0.0, N, alpha)
    for a, b in zip(ref[:4], got[:4]):
        assert a.dtype == b.dtype and _bytes(a) == _bytes(b)
    for k in ref[4]:
        assert _bytes(ref[4][k]) == _bytes(got[4][k]), k
    assert _bytes(got[4]["att"]) == _bytes(ref[3])


def test_joint_decode_batch_and_limits(gpu):
    from onebit_asr.attdec import joint_beam_search
    from onebit_asr.metrics import joint_decode_batch

    model, _ = _decoder_model(35, 64)
    enc, mask = _memory(0, 64, LENS, gpu)
    with torch.no_grad():
        z = model.ctc_logits(enc)
    hyp, hyp_len, _, _, _ = joint_beam_search(model, enc, mask, z, 4, 8, 0.3)
    assert joint_decode_batch(model, enc, mask, z, 4, 8, 0.3) == \
        [hyp[b, 0, :hyp_len[b, 0]].tolist() for b in range(3)]
    for kw in (dict(beam_size=4, ctc_cand=3), dict(beam_size=4, ctc_cand=33),
               dict(beam_size=33), dict(beam_size=4, max_len=256)):
        with pytest.raises(ValueError, match="not supported"):
            joint_beam_search(model, enc, mask, z, **kw)
    with pytest.raises(ValueError, match="ctc_weight"):
        joint_beam_search(model, enc, mask, z, 4, 8, 1.5)


# ------------------------------------------------------------------------------------------
# 8. graphed
# ------------------------------------------------------------------------------------------
def test_graphed_joint_search_equals_eager_bitwise(gpu):
    from onebit_asr.conformer import ConformerASR
    from onebit_asr.data import CFG1, synthetic_batch
    from onebit_asr.infer import GraphedInference, encode_and_decode
    from onebit_asr.quant import set_act_quant

    torch.manual_seed(0)
    model = ConformerASR(80, 5004, **CFG1).to(gpu).eval()
    feat_lens, tok_lens = [349, 61], [12, 3]
    b1 = synthetic_batch(feat_lens, tok_lens, seed=0, device=gpu)
    b2 = synthetic_batch(feat_lens, tok_lens, seed=1, device=gpu)
    gi = GraphedInference(model, act_quant=None, decoder="attention", beam_size=4, max_len=12,
                          joint_ctc_weight=0.3)
    keys = ("hyp", "hyp_len", "n_hyp", "score", "finished", "trace_parent", "trace_token",
            "trace_score", "att", "ctc")
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
                                        info=info, joint_ctc_weight=0.3)
        assert out.shape == (2, 12) and out.dtype == cnt.dtype == torch.int32
        assert torch.equal(out, info["hyp"][:, 0]) and torch.equal(cnt, info["hyp_len"][:, 0])
        eager.append((out, cnt, info))

    def same(run, ref):
        assert torch.equal(run[0], ref[0]) and torch.equal(run[1], ref[1])
        for k in keys:
            assert _bytes(run[2][k]) == _bytes(ref[2][k]), k

    same(runs[0], eager[0])
    same(runs[1], runs[0])
    same(runs[3], runs[0])
    same(runs[2], eager[1])
    # the joint search is not the attention-only search
    info0 = {}
    encode_and_decode(model, b1, decoder="attention", beam_size=4, max_len=12, info=info0)
    assert "att" not in info0
    assert _bytes(info0["score"]) != _bytes(eager[0][2]["score"])
