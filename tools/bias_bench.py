#!/usr/bin/env python3
"""Contextual-biasing timing: the CTC prefix beam search with the phrase automaton inside it
(``ctc_beam_search_bias_device``, ob_ctc_beam_search_bias) next to the searches it extends, and the
biased attention beam step next to the fused step.

Eval shape: B = 32, T' = 249, V = 5004, beam 10, the 20 best tokens per frame, 1000 random phrases
of 1..6 tokens, the 200k-entry order-4 table of tests/ngram_ref.big_lm; synthetic CTC-like logits
(tools/decode_bench.py's). HIP events around each call on the launch stream after warm-up, the
median and the spread over --reps replays of a captured graph, the whole set --repeat times (the
run-to-run spread):

* ``one_best`` / ``nbest`` / ``lm``   the three existing instantiations of the search kernel;
* ``bias`` / ``bias_lm``              the two new ones (without and with the LM).

``--mode existing`` times the first three only and imports nothing new, so that ``--root DIR``
can point it at another checkout of this repository (its package and library), e.g. the parent
commit's, for the parent's own run-to-run spread.

``--mode step``: the attention side. A joint search with an LM is run phase by phase on a decoder
of Conformer-S size; at three steps ``ob_attdec_fused_step`` and ``ob_attdec_biased_step`` are timed
on copies of the state the search has, and ``ob_bias_step`` next to ``ob_ngram_step``.
One JSON line. Usage: python tools/bias_bench.py [--mode all|existing|step] [--root DIR]"""
import argparse
import json
import sys
from pathlib import Path
from types import SimpleNamespace

HERE = Path(__file__).resolve().parents[1]
ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("all", "existing", "step"), default="all")
ap.add_argument("--root", default=str(HERE))
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--frames", type=int, default=249)
ap.add_argument("--vocab", type=int, default=5004)
ap.add_argument("--beam", type=int, default=10)
ap.add_argument("--top-k", type=int, default=20)
ap.add_argument("--phrases", type=int, default=1000)
ap.add_argument("--bias-weight", type=float, default=1.0)
ap.add_argument("--lm-weight", type=float, default=0.5)
args = ap.parse_args()
ROOT = Path(args.root).resolve()
sys.path[:0] = [str(ROOT), str(ROOT / "cmu-11785-idl-1.58bit-asr_amd"), str(ROOT / "tools"),
                str(ROOT / "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import onebit_asr  # noqa: E402,F401  (ahead of decode_bench, which puts its own tree on the path)
from onebit_asr import _lib  # noqa: E402
from decode_bench import ctc_like_logits, timed  # noqa: E402
from onebit_asr.infer import (ctc_beam_search_batch_device, ctc_beam_search_lm_device,  # noqa: E402
                              ctc_beam_search_nbest_device)

BLANK = 3


def graphed(fn, reps, warmup):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()
    res = timed(graph.replay, reps, warmup)
    del graph, keep
    return res


def random_phrases(count, V, seed):
    rng = np.random.default_rng(seed)
    return [([int(t) for t in rng.integers(4, V, size=int(rng.integers(1, 7)))],
             float(rng.choice([0.5, 1.0, 2.0]))) for _ in range(count)]


def searches(dev):
    B, T, V, beam, top_k = args.batch, args.frames, args.vocab, args.beam, args.top_k
    from ngram_ref import big_lm
    from onebit_asr.ngram import NGramLM

    ref, ids, n, vals = big_lm(V=V)
    lm = NGramLM.from_arrays(ids, n, vals, ref.order)
    lm.device_table(dev)
    x, lens = ctc_like_logits(B, T, V, BLANK, 0, dev)
    fns = {"one_best": lambda: ctc_beam_search_batch_device(x, lens, beam, BLANK, top_k),
           "nbest": lambda: ctc_beam_search_nbest_device(x, lens, beam, None, BLANK, top_k),
           "lm": lambda: ctc_beam_search_lm_device(x, lens, lm, args.lm_weight, 0.0, beam, None,
                                                   BLANK, top_k)}
    res = {}
    if args.mode == "all":
        from onebit_asr.bias import ContextBias
        from onebit_asr.infer import ctc_beam_search_bias_device

        ctx = ContextBias(random_phrases(args.phrases, V, 11))
        ctx.device_tables(dev)
        res["automaton"] = {"phrases": ctx.n_phrases, "nodes": ctx.n_nodes, "slots": ctx.slots,
                            "bytes": 16 * (ctx.n_nodes + ctx.slots), "max_probe": ctx.max_probe}
        fns["bias"] = lambda: ctc_beam_search_bias_device(
            x, lens, ctx, args.bias_weight, None, 0.0, 0.0, beam, None, BLANK, top_k)
        fns["bias_lm"] = lambda: ctc_beam_search_bias_device(
            x, lens, ctx, args.bias_weight, lm, args.lm_weight, 0.0, beam, None, BLANK, top_k)
    for name, fn in fns.items():
        runs = [graphed(fn, args.reps, args.warmup) for _ in range(args.repeat)]
        med = [r["median_us"] for r in runs]
        res[name] = {"medians_us": med, "median_us": sorted(med)[len(med) // 2],
                     "spread_us": round(max(med) - min(med), 1),
                     "min_us": min(r["min_us"] for r in runs),
                     "max_us": max(r["max_us"] for r in runs)}
        print(name, res[name], file=sys.stderr, flush=True)
    if args.mode == "all":
        hyp, hyp_len, _, info = fns["bias"]()
        p_hyp, p_len, _, _ = fns["nbest"]()
        res["utterances_with_another_best"] = int(sum(
            hyp[b, 0, :hyp_len[b, 0]].tolist() != p_hyp[b, 0, :p_len[b, 0]].tolist()
            for b in range(B)))
        res["bias_over_nbest"] = round(res["bias"]["median_us"] / res["nbest"]["median_us"], 3)
        res["bias_lm_over_lm"] = round(res["bias_lm"]["median_us"] / res["lm"]["median_us"], 3)
    res["frames_total"] = int(lens.sum().item())
    return res


@torch.no_grad()
def step(dev):
    from ngram_ref import big_lm
    from onebit_asr.attdec import SPECIAL, _BeamSearch
    from onebit_asr.bias import ContextBias, bias_step
    from onebit_asr.conformer import TransformerDecoder
    from onebit_asr.data import CONFORMER_S
    from onebit_asr.ngram import NGramLM, ngram_step

    B, T, V, N, K, L = args.batch, args.frames, args.vocab, args.beam, 2 * args.beam, 32
    d = CONFORMER_S["enc_d_model"]
    ref, ids, n, vals = big_lm(V=V)
    lm = NGramLM.from_arrays(ids, n, vals, ref.order)
    ctx = ContextBias(random_phrases(args.phrases, V, 11))
    z, lens = ctc_like_logits(B, T, V, BLANK, 0, dev)
    torch.manual_seed(0)
    dec = TransformerDecoder(V, d, CONFORMER_S["dec_layers"], CONFORMER_S["dec_heads"],
                             CONFORMER_S["dec_d_ff"], 0.1, 0).to(dev).eval()
    model = SimpleNamespace(decoder=dec)
    g = torch.Generator().manual_seed(1)
    mem = torch.randn(B, T, d, generator=g).to(dev)
    mask = (torch.arange(T)[None, :] < lens.cpu().clamp(min=1)[:, None]).to(dev)
    out = {}
    for name, bias in (("fused", None), ("biased", ctx)):
        bs = _BeamSearch(model, mem, mask, N, K, L, 0.0, SPECIAL, z, 0.3, lm, args.lm_weight, bias,
                         args.bias_weight)
        st = bs.state
        for t in range(L):
            bs.propose(t)
            bs.score_ctc(t)
            bs.score_lm(t)
            if bias is not None:
                bs.score_bias(t)
            if t in (0, L // 2 - 1, L - 1):
                moved = ("score", "att", "ctc", "lm", "bias", "length", "fin", "tok", "skip",
                         "link", "anc", "trace")
                copy = bs.clone_state(moved)
                out[f"{name}_step_t{t}"] = timed(lambda: bs.select(t, copy), args.reps,
                                                 args.warmup)
                if bias is not None:
                    s_st, s_kept = torch.zeros_like(st["bst"][0]), torch.zeros_like(st["bkept"][0])
                    s_sc = torch.empty_like(st["bsc"])
                    out[f"bias_step_t{t}"] = timed(lambda: bias_step(
                        ctx, st["cand"][2], st["tok"], st["length"], st["link"], st["skip"],
                        st["bst"][t & 1], s_st, st["bkept"][t & 1], s_kept, s_sc, N,
                        SPECIAL["eos"]), args.reps, args.warmup)
                    s_ctx, l_sc = torch.zeros_like(st["lmctx"][0]), torch.empty_like(st["lmsc"])
                    out[f"ngram_step_t{t}"] = timed(lambda: ngram_step(
                        lm, st["cand"][2], st["tok"], st["length"], st["link"], st["skip"],
                        st["lmctx"][t & 1], s_ctx, l_sc, N, V), args.reps, args.warmup)
                    out[f"live_rows_t{t}"] = int((st["skip"] == 0).sum().item())
            bs.select(t)
    return out


def main():
    dev = torch.device("cuda:0")
    res = step(dev) if args.mode == "step" else searches(dev)
    print(json.dumps({"tool": "bias_bench", "mode": args.mode, "root": ROOT.name,
                      "device": torch.cuda.get_device_name(0), "B": args.batch, "T": args.frames,
                      "V": args.vocab, "beam": args.beam, "top_k": args.top_k, "reps": args.reps,
                      "repeat": args.repeat, **res, "digest": _lib.source_digest()[:12]}))


if __name__ == "__main__":
    main()
