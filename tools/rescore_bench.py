#!/usr/bin/env python3
"""Two-pass decoding timing at the inference batch (B = 256, T' = 249, V = 5004, d = 144,
N = 10 hypotheses per utterance, ragged lengths, hypothesis lengths of about 10 to 60 at the
static length 64). HIP events around each call on the launch stream, after warm-up; the median
and the spread over --reps calls. Reports, as one JSON line:

* the n-best beam search next to the 1-best search (seeded CTC-like logits, as decode_bench.py);
* the decoder over the n-best with shared encoder memory (``TransformerDecoder.hidden``,
  mem_group = N), next to the same on ``repeat_interleave``d memory through ``forward``'s path;
* the fused scorer (``ob_seq_logprob``) next to the unfused expression it replaces (``linear``
  -> ``log_softmax`` -> ``gather`` in torch on the same inputs), and their largest difference;
* the whole ``decoder="rescore"`` forward next to ``decoder="beam"`` (Conformer-S, captured
  graphs, int8 activations). The model is untrained, so its CTC head emits a token on almost
  every frame; the tool shifts the blank bias until about 15% of the frames are non-blank, so
  that hypotheses have the lengths a trained model gives and fit max_len = 64 (the share of
  utterances that were rescored is reported).
Usage: python tools/rescore_bench.py [--reps 20] [--skip-forward]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "cmu-11785-idl-1.58bit-asr_amd"), str(ROOT / "tools")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from decode_bench import ctc_like_logits, timed  # noqa: E402
from onebit_asr import _lib  # noqa: E402
from onebit_asr.conformer import ConformerASR, TransformerDecoder  # noqa: E402
from onebit_asr.data import CONFORMER_S, synthetic_batch  # noqa: E402
from onebit_asr.infer import (GraphedInference, ctc_beam_search_batch_device,  # noqa: E402
                              ctc_beam_search_nbest_device, seq_logprob)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--vocab", type=int, default=5004)
    ap.add_argument("--nbest", type=int, default=10)
    ap.add_argument("--max-len", type=int, default=64)
    ap.add_argument("--skip-forward", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, T, V, N, Lc = args.batch, args.frames, args.vocab, args.nbest, args.max_len
    d = CONFORMER_S["enc_d_model"]
    res = {}

    # 1. the search
    x, lens = ctc_like_logits(B, T, V, 3, 0, dev)
    res["beam_1best"] = timed(lambda: ctc_beam_search_batch_device(x, lens, N, 3), args.reps,
                              args.warmup)
    res["beam_nbest"] = timed(lambda: ctc_beam_search_nbest_device(x, lens, N, N, 3), args.reps,
                              args.warmup)
    del x

    # 2. the decoder over the n-best: seeded memory, ragged masks, hypothesis lengths 10..60
    torch.manual_seed(0)
    dec = TransformerDecoder(V, d, CONFORMER_S["dec_layers"], CONFORMER_S["dec_heads"],
                             CONFORMER_S["dec_d_ff"], 0.1, 0).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    mem = torch.randn(B, T, d, generator=g).to(dev)
    mask = (torch.arange(T)[None, :] < lens.cpu()[:, None]).to(dev)
    hl = torch.randint(10, 61, (B * N,), generator=g)
    pos = torch.arange(Lc + 1)[None, :]
    toks = torch.randint(4, V, (B * N, Lc + 1), generator=g)
    tgt_inp = torch.where(pos == 0, torch.tensor(1), torch.where(pos <= hl[:, None], toks,
                                                                 torch.tensor(0))).to(dev)
    target = torch.where(pos < hl[:, None], toks.roll(-1, 1),
                         torch.where(pos == hl[:, None], torch.tensor(2), torch.tensor(-1)))
    target = target.to(torch.int32).to(dev)
    tgt_pad = (pos > hl[:, None]).to(dev)
    live_rows = int((target >= 0).sum().item())
    res["decoder_shared_memory"] = timed(
        lambda: dec.hidden(tgt_inp, mem, mask, tgt_pad, mem_group=N), args.reps, args.warmup)
    mem_rep, mask_rep = mem.repeat_interleave(N, 0), mask.repeat_interleave(N, 0)
    res["decoder_repeated_memory"] = timed(
        lambda: dec.hidden(tgt_inp, mem_rep, mask_rep, tgt_pad, mem_group=1), args.reps,
        args.warmup)
    del mem_rep, mask_rep

    # 3. the scorer, fused and unfused, on the decoder's hidden states
    with torch.no_grad():
        h = dec.hidden(tgt_inp, mem, mask, tgt_pad, mem_group=N).reshape(-1, d).contiguous()
        w, bias = dec.out.weight.detach(), dec.out.bias.detach()
        tg = target.reshape(-1)
        res["scorer_fused"] = timed(lambda: seq_logprob(h, w, bias, tg), args.reps, args.warmup)
        idx = tg.clamp(min=0).long().unsqueeze(1)

        def unfused():
            lsm = torch.log_softmax(F.linear(h, w, bias), dim=-1)
            return lsm.gather(1, idx).squeeze(1).masked_fill(tg < 0, 0.0)

        res["scorer_unfused_torch"] = timed(unfused, max(3, args.reps // 4), 2)
        diff = float((seq_logprob(h, w, bias, tg) - unfused()).abs().max().item())
    rows = h.shape[0]
    res["scorer_workspace_bytes"] = lib.ob_seq_logprob_workspace(rows, d, V)
    res["unfused_logits_bytes"] = rows * V * 4
    del h, mem

    # 4. the whole forward, captured
    fwd = {}
    if not args.skip_forward:
        torch.manual_seed(0)
        model = ConformerASR(80, V, **CONFORMER_S).to(dev).eval()
        batch = synthetic_batch([1000] * B, [40] * B, seed=1234, device=dev)
        batch["feat_lens"] = (lens * 4).clamp(max=1000).to(dev)
        with torch.no_grad():
            _, _, lg = model(batch, precision=2)
            others = lg.clone()
            others[..., 3] = -float("inf")
            gap = (others.max(dim=-1).values - lg[..., 3]).flatten()
            model.ctc_head.bias[3] += torch.quantile(gap[:1 << 20].float(), 0.85)
            del lg, others, gap
        for name in ("beam", "rescore"):
            gi = GraphedInference(model, precision=2, decoder=name, beam_size=N, max_len=Lc)
            gi.run(batch)
            fwd["forward_" + name] = timed(lambda: gi.run(batch), max(3, args.reps // 2), 1)
            if name == "rescore":
                torch.cuda.synchronize()
                hlen = gi.info["hyp_len"][:, 0].float()
                fwd["rescored_share"] = round(float(gi.info["rescored"].float().mean().item()), 3)
                fwd["best_hyp_len_mean_max"] = [round(float(hlen.mean().item()), 1),
                                                int(hlen.max().item())]
                fwd["winner_is_not_ctc_best"] = int((gi.info["best_k"] != 0).sum().item())
            del gi
    print(json.dumps({"tool": "rescore_bench", "device": torch.cuda.get_device_name(0), "B": B,
                      "T": T, "V": V, "d": d, "nbest": N, "max_len": Lc, "rows": rows,
                      "live_rows": live_rows, "reps": args.reps, **res,
                      "fused_vs_unfused_max_abs_diff": diff, **fwd,
                      "digest": _lib.source_digest()[:12]}))


if __name__ == "__main__":
    main()
