#!/usr/bin/env python3
"""N-gram LM shallow fusion timing (B = 32, N = 10 beam slots, K = 20 candidates per slot,
T' = 250, V = 5004, L = 64 static steps, order 4; random tables of --entries entries, default 2e5
and 4e6, the second larger than L2). HIP events around each call on the launch stream, after
warm-up; the median and the spread over --reps calls. One JSON line.

--mode all (default):
* ``ob_ngram_step`` per launch on the fused search's own state at steps 0, 31 and 63, next to
  ``ob_ctc_prefix_step`` at the same shape and steps from the same run; the table slots examined
  per candidate (mean, max) for those steps' (context, candidate) pairs, from the host scorer
  (``ob_ngram_score_host``), which runs the kernels' probe routine;
* ``joint_beam_search`` with and without the LM, eager and replayed from a captured graph;
* ``ob_ngram_seq_logprob`` on a [320][64] n-best, next to ``attention_rescore`` (the decoder pass,
  the output-layer scorer and the pick) on the same n-best with and without the LM.
--mode joint-base: ``joint_beam_search`` without an LM only, --repeat times in one process; with
--root pointing at another checkout (e.g. the parent commit, built) this times that tree's search
at the same arguments, for an A/B against this one.
--mode steps: the first item only (for a run under ``rocprofv3 --kernel-trace --stats``, which
gives the kernels' own times without the launch path).
Usage: python tools/ngram_bench.py [--reps 20] [--mode all|joint-base|steps] [--root DIR]"""
import argparse
import json
import sys
from pathlib import Path
from types import SimpleNamespace

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--mode", default="all", choices=("all", "joint-base", "steps"))
ap.add_argument("--root", default=None)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--entries", type=int, nargs="*", default=[200_000, 4_000_000])
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--frames", type=int, default=250)
ap.add_argument("--vocab", type=int, default=5004)
ap.add_argument("--beam", type=int, default=10)
ap.add_argument("--cand", type=int, default=20)
ap.add_argument("--max-len", type=int, default=64)
ap.add_argument("--weight", type=float, default=0.3)
ap.add_argument("--lm-weight", type=float, default=0.5)
args = ap.parse_args()

HERE = Path(__file__).resolve().parents[1]
ROOT = Path(args.root).resolve() if args.root else HERE
sys.path[:0] = [str(ROOT), str(ROOT / "cmu-11785-idl-1.58bit-asr_amd"), str(HERE / "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import onebit_asr  # noqa: E402  (ahead of decode_bench, which puts its own tree on the path)
from onebit_asr import _lib  # noqa: E402
from decode_bench import ctc_like_logits, timed  # noqa: E402
from onebit_asr.attdec import joint_beam_search  # noqa: E402
from onebit_asr.conformer import TransformerDecoder  # noqa: E402
from onebit_asr.data import CONFORMER_S  # noqa: E402

PAD, BOS, EOS, BLANK = 0, 1, 2, 3


def random_table(n_entries, V, seed):
    """ids [E, 4], n [E], vals [E, 2] of a random order-4 model: every word's unigram, then equal
    shares of 2-, 3- and 4-grams, each extending an n-gram of the order below."""
    rng = np.random.default_rng(seed)
    words = np.array([v for v in range(V) if v not in (PAD, BLANK)], np.int64)
    grams = [words[:, None]]
    per = (n_entries - len(words)) // 3
    for n in range(2, 5):
        prev = grams[-1][grams[-1][:, -1] != EOS]
        ext = np.concatenate([prev[rng.integers(0, len(prev), size=2 * per)],
                              rng.choice(words[words != BOS], size=2 * per)[:, None]], axis=1)
        ext = np.unique(ext, axis=0)
        rng.shuffle(ext)
        grams.append(ext[:per])
    e = sum(len(g) for g in grams)
    ids = np.zeros((e, 4), np.int64)
    n_arr = np.zeros(e, np.int64)
    o = 0
    for g in grams:
        ids[o:o + len(g), :g.shape[1]] = g
        n_arr[o:o + len(g)] = g.shape[1]
        o += len(g)
    vals = np.stack([-rng.uniform(0.1, 9.0, size=e), -rng.uniform(0.0, 2.0, size=e)],
                    axis=1).astype(np.float32)
    return ids, n_arr, vals


@torch.no_grad()
def stepwise(model, enc, mask, z, lms, n, k, L, w, lw, keep, reps, warmup):
    """The fused search with the first LM of ``lms``, phase by phase (``attdec._BeamSearch``); at
    the steps in ``keep`` the LM step of every table and the CTC scorer step are timed on the
    state the search has."""
    from onebit_asr.attdec import SPECIAL, _BeamSearch  # (here: --root may be an older tree)
    from onebit_asr.ngram import ngram_step

    bs = _BeamSearch(model, enc, mask, n, k, L, 0.0, SPECIAL, z, w, lms[0][1], lw)
    assert bs.mode.ctc and bs.mode.lm, "--weight and --lm-weight must be > 0: both are timed"
    st = bs.state
    v = model.decoder.out.weight.shape[0]
    scratch_ctx = torch.zeros_like(st["lmctx"][0])
    scratch_sc = torch.empty_like(st["lmsc"])
    out = {}
    for t in range(L):
        bs.propose(t)
        bs.score_ctc(t)
        bs.score_lm(t)
        if t in keep:
            out[f"ctc_prefix_step_t{t}"] = timed(lambda: bs.score_ctc(t), reps, warmup)
            topi, skip = st["cand"][2], st["skip"]
            c_in, c_out = st["lmctx"][t & 1], st["lmctx"][(t + 1) & 1]
            live = (skip == 0).cpu().numpy()
            ctx_h = np.repeat(c_out.cpu().numpy().astype(np.uint64)[live], k)
            w_h = topi.cpu().numpy()[live].reshape(-1)
            for name, lm in lms:
                out[f"ngram_step_{name}_t{t}"] = timed(
                    lambda: ngram_step(lm, topi, st["tok"], st["length"], st["link"], skip, c_in,
                                       scratch_ctx, scratch_sc, n, v), reps, warmup)
                _, pr = lm.score_host(ctx_h, w_h, v, probes=True)
                out[f"probes_per_candidate_{name}_t{t}"] = {
                    "mean": round(float(pr.mean()), 2), "max": int(pr.max()),
                    "candidates": int(len(pr))}
                out[f"ngram_over_ctc_{name}_t{t}"] = round(
                    out[f"ngram_step_{name}_t{t}"]["median_us"] /
                    out[f"ctc_prefix_step_t{t}"]["median_us"], 4)
            out[f"live_rows_t{t}"] = int(live.sum())
        bs.select(t)
    return out


def main():
    dev = torch.device("cuda:0")
    B, T, V, N, K, L, w, lw = (args.batch, args.frames, args.vocab, args.beam, args.cand,
                               args.max_len, args.weight, args.lm_weight)
    d = CONFORMER_S["enc_d_model"]
    res = {}

    def note(msg):
        print(msg, file=sys.stderr, flush=True)

    z, lens = ctc_like_logits(B, T, V, BLANK, 0, dev)
    torch.manual_seed(0)
    dec = TransformerDecoder(V, d, CONFORMER_S["dec_layers"], CONFORMER_S["dec_heads"],
                             CONFORMER_S["dec_d_ff"], 0.1, 0).to(dev).eval()
    model = SimpleNamespace(decoder=dec)
    g = torch.Generator().manual_seed(1)
    mem = torch.randn(B, T, d, generator=g).to(dev)
    mask = (torch.arange(T)[None, :] < lens.cpu().clamp(min=1)[:, None]).to(dev)

    def time_search(fn, name):
        res[f"{name}_eager"] = timed(fn, args.reps, args.warmup)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fn()
        res[f"{name}_graph"] = timed(graph.replay, args.reps, args.warmup)
        note(f"{name}: eager {res[f'{name}_eager']} graph {res[f'{name}_graph']}")
        del graph, out

    head = {"tool": "ngram_bench", "mode": args.mode, "root": str(ROOT.name),
            "package": str(Path(onebit_asr.__file__).resolve().parents[2].name),
            "device": torch.cuda.get_device_name(0), "B": B, "T": T, "V": V, "d": d, "beam": N,
            "cand": K, "max_len": L, "weight": w, "rows": B * N, "reps": args.reps}
    if args.mode == "joint-base":
        for i in range(args.repeat):
            time_search(lambda: joint_beam_search(model, mem, mask, z, N, L, w, K), f"joint_nolm_{i}")
        print(json.dumps({**head, **res, "digest": _lib.source_digest()[:12]}))
        return

    from onebit_asr.infer import attention_rescore
    from onebit_asr.ngram import NGramLM, ngram_seq_logprob

    lms = []
    for e in args.entries:
        lm = NGramLM.from_arrays(*random_table(e, V, 7), 4)
        lm.device_table(dev)
        name = f"{e // 1000}k"
        lms.append((name, lm))
        res[f"table_{name}"] = {"entries": lm.n_entries, "slots": lm.slots,
                                "bytes": lm.slots * 16, "max_probe": lm.max_probe}
        note(f"table {name}: {res[f'table_{name}']}")

    res.update(stepwise(model, mem, mask, z, lms, N, K, L, w, lw, (0, L // 2 - 1, L - 1),
                        args.reps, args.warmup))
    if args.mode == "steps":        # (the kernels alone, e.g. under a kernel trace)
        print(json.dumps({**head, **res, "digest": _lib.source_digest()[:12]}))
        return
    for i in range(args.repeat):
        time_search(lambda: joint_beam_search(model, mem, mask, z, N, L, w, K), f"joint_nolm_{i}")
    for name, lm in lms:
        time_search(lambda: joint_beam_search(model, mem, mask, z, N, L, w, K, lm=lm,
                                              lm_weight=lw), f"joint_lm_{name}")
        res[f"lm_added_us_per_search_{name}"] = {
            kind: round(res[f"joint_lm_{name}_{kind}"]["median_us"] -
                        res[f"joint_nolm_0_{kind}"]["median_us"], 1) for kind in ("eager", "graph")}

    # a [B * N][L] n-best of full-length hypotheses
    rng = np.random.default_rng(3)
    hyp = torch.from_numpy(rng.integers(4, V, size=(B, N, L)).astype(np.int32)).to(dev)
    hyp_len = torch.full((B, N), L, dtype=torch.int32, device=dev)
    n_hyp = torch.full((B,), N, dtype=torch.int32, device=dev)
    ctc_sc = torch.zeros((B, N), dtype=torch.float64, device=dev)
    for name, lm in lms:
        res[f"ngram_seq_logprob_{name}"] = timed(lambda: ngram_seq_logprob(lm, hyp, hyp_len, V),
                                                 args.reps, args.warmup)
    res["attention_rescore_nolm"] = timed(
        lambda: attention_rescore(model, mem, mask, hyp, hyp_len, n_hyp, ctc_sc, 0.5, L),
        args.reps, args.warmup)
    for name, lm in lms:
        res[f"attention_rescore_lm_{name}"] = timed(
            lambda: attention_rescore(model, mem, mask, hyp, hyp_len, n_hyp, ctc_sc, 0.5, L,
                                      lm=lm, lm_weight=lw), args.reps, args.warmup)
    print(json.dumps({**head, **res, "digest": _lib.source_digest()[:12]}))


if __name__ == "__main__":
    main()
