#!/usr/bin/env python3
"""First-pass LM fusion timing: the CTC prefix beam search with the n-gram LM inside it
(``ctc_beam_search_lm_device``, ob_ctc_beam_search_lm) next to what it replaces and to the encoder.

Eval shape: B = 32, T' = 249, V = 5004, beam 10, the 20 best tokens per frame, the 200k-entry
order-4 table of tests/ngram_ref.big_lm; synthetic CTC-like logits (tools/decode_bench.py's). HIP
events around each call on the launch stream after warm-up, the median and the spread over --reps
calls, eager (allocations and launch path included) and replayed from a captured graph:

* ``fused``     ctc_beam_search_lm_device, nbest = beam;
* ``baseline``  ctc_beam_search_nbest_device + ctc_lm_rescore (LM re-ranking of the plain n-best);
* ``plain``     ctc_beam_search_nbest_device alone (the search without any LM);
* ``encoder``   the Conformer-S encoder + CTC head forward the decoders share (2-bit weights, int8
                activations), B x 1000 frames, for scale.

Also: how many utterances change their best hypothesis under fusion. One JSON line.
Usage: python tools/beam_lm_bench.py [--reps 30] [--warmup 5]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "cmu-11785-idl-1.58bit-asr_amd"), str(ROOT / "tools"),
                str(ROOT / "tests")]

import torch  # noqa: E402

from decode_bench import ctc_like_logits, timed  # noqa: E402
from onebit_asr import _lib  # noqa: E402
from onebit_asr.infer import (ctc_beam_search_lm_device, ctc_beam_search_nbest_device,  # noqa: E402
                              ctc_lm_rescore)

BLANK = 3


def both(fn, reps, warmup):
    """-> {eager, graph}: the call as it stands, and replayed from a captured graph."""
    eager = timed(fn, reps, warmup)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()
    res = {"eager": eager, "graph": timed(graph.replay, reps, warmup)}
    del graph, keep
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--vocab", type=int, default=5004)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--top-k", type=int, default=20)
    ap.add_argument("--lm-weight", type=float, default=0.5)
    ap.add_argument("--ins-bonus", type=float, default=0.0)
    ap.add_argument("--no-encoder", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, T, V, beam, top_k = args.batch, args.frames, args.vocab, args.beam, args.top_k

    from ngram_ref import big_lm
    from onebit_asr.ngram import NGramLM

    ref, ids, n, vals = big_lm(V=V)
    lm = NGramLM.from_arrays(ids, n, vals, ref.order)
    lm.device_table(dev)
    x, lens = ctc_like_logits(B, T, V, BLANK, 0, dev)

    def fused():
        return ctc_beam_search_lm_device(x, lens, lm, args.lm_weight, args.ins_bonus, beam, None,
                                         BLANK, top_k)

    def plain():
        return ctc_beam_search_nbest_device(x, lens, beam, None, BLANK, top_k)

    def baseline():
        hyp, hyp_len, n_hyp, score = plain()
        return ctc_lm_rescore(hyp, hyp_len, n_hyp, score, lm, args.lm_weight, V)

    res = {"fused": both(fused, args.reps, args.warmup),
           "baseline": both(baseline, args.reps, args.warmup),
           "plain": both(plain, args.reps, args.warmup)}
    frames = int(lens.max().item())
    res["fused_us_per_frame_longest"] = round(res["fused"]["graph"]["median_us"] / frames, 2)
    res["fused_over_baseline"] = round(res["fused"]["graph"]["median_us"] /
                                       res["baseline"]["graph"]["median_us"], 3)
    hyp, hyp_len, _, info = fused()
    out, cnt, _ = baseline()
    changed = sum(hyp[b, 0, :hyp_len[b, 0]].tolist() != out[b, :cnt[b]].tolist() for b in range(B))
    res["utterances_with_another_best"] = int(changed)

    if not args.no_encoder:
        from onebit_asr.conformer import ConformerASR
        from onebit_asr.data import CONFORMER_S, synthetic_batch
        from onebit_asr.quant import set_act_quant

        torch.manual_seed(0)
        model = ConformerASR(80, V, **CONFORMER_S).to(dev).eval()
        set_act_quant(model, "absmax_int8")
        batch = synthetic_batch([1000] * B, [40] * B, vocab=V, seed=1234, device=dev)
        with torch.no_grad():
            enc = both(lambda: model(batch, precision=2), args.reps, args.warmup)
            t_enc = model(batch, precision=2)[2].shape[1]
        res["encoder"] = enc
        res["encoder_frames_out"] = int(t_enc)
        res["fused_over_encoder"] = round(res["fused"]["graph"]["median_us"] /
                                          enc["graph"]["median_us"], 3)
    print(json.dumps({"tool": "beam_lm_bench", "device": torch.cuda.get_device_name(0), "B": B,
                      "T": T, "V": V, "beam": beam, "top_k": top_k, "lm_weight": args.lm_weight,
                      "ins_bonus": args.ins_bonus, "frames_total": int(lens.sum().item()),
                      "table": {"entries": lm.n_entries, "slots": lm.slots,
                                "bytes": lm.slots * 16, "max_probe": lm.max_probe,
                                "order": lm.order},
                      "reps": args.reps, **res, "digest": _lib.source_digest()[:12]}))


if __name__ == "__main__":
    main()
