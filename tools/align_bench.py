#!/usr/bin/env python3
"""CTC forced alignment timing at decode_bench.py's shape (B = 256, T' = 249, V = 5004, CTC-like
logits, ragged lengths). The targets are the greedy decode of the same logits, cut to S tokens
(always alignable), at S = 64 and at S = T' (the greedy output's width). HIP events around each
call on the launch stream, after warm-up; the median and the spread over --reps calls. Reports,
as one JSON line and per S:

* the whole call (``ob_ctc_align``), and its phases through ``ob_ctc_align_stage``: the emission
  launch, the trellis launch, the trellis launch without its walk (the recursion alone), and the
  walk + outputs as the difference of the two;
* the workspace in bytes and the logits bytes the emission launch reads, with the rate that is;
* for scale, on the same logits: ``ob_ctc_frame_lse`` and ``ob_ctc_beam_search``.
Usage: python tools/align_bench.py [--reps 30]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "cmu-11785-idl-1.58bit-asr_amd"), str(ROOT / "tools")]

import torch  # noqa: E402

from decode_bench import ctc_like_logits, timed  # noqa: E402
from onebit_asr import _lib  # noqa: E402
from onebit_asr.align import ctc_forced_align  # noqa: E402
from onebit_asr.attdec import ctc_frame_lse  # noqa: E402
from onebit_asr.infer import ctc_beam_search_batch_device, ctc_greedy_decode_batch  # noqa: E402

BLANK = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--vocab", type=int, default=5004)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, T, V = args.batch, args.frames, args.vocab
    z, lens = ctc_like_logits(B, T, V, BLANK, 0, dev)
    lens = lens.to(torch.int64).contiguous()
    hyp, cnt = ctc_greedy_decode_batch(z, lens, BLANK)
    st = _lib.stream_of(z)
    res = {}
    for S in sorted({min(64, T), min(T, 511)}):
        tg = hyp[:, :S].contiguous()
        tl = cnt.clamp(max=S).contiguous()
        path = torch.empty((B, T), dtype=torch.int32, device=dev)
        span = torch.empty((B, S, 2), dtype=torch.int32, device=dev)
        tok = torch.empty((B, S), dtype=torch.float64, device=dev)
        score = torch.empty((B,), dtype=torch.float64, device=dev)
        need = lib.ob_ctc_align_workspace(B, T, S)
        ws = torch.empty((need // 8,), dtype=torch.int64, device=dev)

        def stage(k):
            _lib.check(lib.ob_ctc_align_stage(
                z.data_ptr(), lens.data_ptr(), tg.data_ptr(), tl.data_ptr(), B, T, V, S, BLANK, k,
                ws.data_ptr(), need, path.data_ptr(), span.data_ptr(), tok.data_ptr(),
                score.data_ptr(), st), "ob_ctc_align_stage")

        r = {"tlen_mean": round(float(tl.float().mean().item()), 1),
             "workspace_bytes": need,
             "all": timed(lambda: stage(0), args.reps, args.warmup),
             "emission": timed(lambda: stage(1), args.reps, args.warmup),
             "trellis": timed(lambda: stage(2), args.reps, args.warmup),
             "recursion_only": timed(lambda: stage(3), args.reps, args.warmup)}
        r["walk_and_outputs_us"] = round(r["trellis"]["median_us"] -
                                         r["recursion_only"]["median_us"], 1)
        stage(0)
        torch.cuda.synchronize()
        r["aligned_share"] = round(float(torch.isfinite(score).float().mean().item()), 3)
        r["python_call"] = timed(lambda: ctc_forced_align(z, lens, tg, tl, BLANK), args.reps,
                                 args.warmup)
        read = int(lens.sum().item()) * V * 4
        r["logits_bytes_read"] = read
        r["emission_GBps"] = round(read / r["emission"]["median_us"] / 1e3, 1)
        res[f"S{S}"] = r
        print(f"S={S} {r}", file=sys.stderr, flush=True)
    flse = torch.empty((B, T), dtype=torch.float64, device=dev)
    res["frame_lse"] = timed(lambda: ctc_frame_lse(z, lens, flse), args.reps, args.warmup)
    res["ctc_beam_search_beam10"] = timed(
        lambda: ctc_beam_search_batch_device(z, lens, 10, BLANK), args.reps, args.warmup)
    res["ctc_greedy"] = timed(lambda: ctc_greedy_decode_batch(z, lens, BLANK), args.reps,
                              args.warmup)
    print(json.dumps({"tool": "align_bench", "device": torch.cuda.get_device_name(0), "B": B,
                      "T": T, "V": V, "frames_valid": int(lens.sum().item()), "reps": args.reps,
                      **res, "digest": _lib.source_digest()[:12]}))


if __name__ == "__main__":
    main()
