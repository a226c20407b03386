#!/usr/bin/env python3
"""Edit distance, n-best distances and MBR selection timing at decode_bench.py's shape (B = 256,
T' = 249, V = 5004, CTC-like logits, ragged lengths, beam 10). The hypotheses are the n-best of
``ob_ctc_beam_search_nbest`` on those logits (N = beam), the references the greedy decode of the
same logits. HIP events around each call on the launch stream, after warm-up; the median and the
spread over --reps calls. Reports, as one JSON line:

* ``ob_edit_distance`` for the B (reference, best hypothesis) pairs, with and without ``ops``;
* ``ob_nbest_edit_distance`` with ``dpair`` (B * N * (N - 1) / 2 pairs), with ``dref`` / ``ops``, and
  with all three;
* ``ob_mbr_select``, and ``edit.mbr_select`` (the two launches and their allocations);
* for scale, on the same inputs: ``ob_ctc_beam_search_nbest``, and the host path these replace,
  ``.cpu()`` plus ``metrics.levenshtein_distance`` over the same B pairs (host clock, copy included)
  and over the pairs of the first --host-utts utterances' n-best (per pair, and scaled to all);
* unless --skip-forward: Conformer-S forward + "beam" decode as one HIP graph, ``mbr_scale=None``
  against ``mbr_scale=1.0``, alternating, and the difference.
Usage: python tools/edit_bench.py [--reps 30] [--out profiles/r14/edit_bench.json]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "cmu-11785-idl-1.58bit-asr_amd"), str(ROOT / "tools")]

import torch  # noqa: E402

from decode_bench import ctc_like_logits, timed  # noqa: E402
from onebit_asr import _lib  # noqa: E402
from onebit_asr.edit import mbr_select  # noqa: E402
from onebit_asr.infer import (GraphedInference, ctc_beam_search_nbest_device,  # noqa: E402
                              ctc_greedy_decode_batch)
from onebit_asr.metrics import levenshtein_distance  # noqa: E402

BLANK = 3


def host_clock(fn, reps):
    """us per call on the host clock (the call ends with the data on the host)."""
    us = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        us.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1),
            "max_us": round(max(us), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--vocab", type=int, default=5004)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--host-utts", type=int, default=16)
    ap.add_argument("--skip-forward", action="store_true")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, T, V, N = args.batch, args.frames, args.vocab, args.beam
    z, lens = ctc_like_logits(B, T, V, BLANK, 0, dev)
    lens = lens.to(torch.int64).contiguous()
    ref, ref_len = ctc_greedy_decode_batch(z, lens, BLANK)
    hyp, hyp_len, n_hyp, score = ctc_beam_search_nbest_device(z, lens, N, None, BLANK)
    best, best_len = hyp[:, 0].contiguous(), hyp_len[:, 0].contiguous()
    st = _lib.stream_of(z)
    i32 = dict(dtype=torch.int32, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    dist, ops = torch.empty((B,), **i32), torch.empty((B, 3), **i32)
    dref, ops_ref = torch.empty((B, N), **i32), torch.empty((B, N, 3), **i32)
    dpair = torch.empty((B, N, N), **i32)
    out, out_len, best_k = torch.empty((B, T), **i32), torch.empty((B,), **i32), torch.empty((B,), **i32)
    risk, post = torch.empty((B, N), **f64), torch.empty((B, N), **f64)
    need = lib.ob_edit_distance_workspace(B, T, T)
    need_n = lib.ob_nbest_edit_distance_workspace(B, N, T, T)
    ws = torch.empty((max(need, need_n) // 8,), dtype=torch.int64, device=dev)

    def pairs(with_ops):
        _lib.check(lib.ob_edit_distance(
            ref.data_ptr(), ref_len.data_ptr(), best.data_ptr(), best_len.data_ptr(), B, T, T,
            ws.data_ptr(), need, dist.data_ptr(), ops.data_ptr() if with_ops else None, st),
            "ob_edit_distance")

    def nbest(with_ref, with_pair):
        _lib.check(lib.ob_nbest_edit_distance(
            hyp.data_ptr(), hyp_len.data_ptr(), n_hyp.data_ptr(), ref.data_ptr(),
            ref_len.data_ptr(), B, N, T, T, ws.data_ptr(), need_n,
            dref.data_ptr() if with_ref else None, ops_ref.data_ptr() if with_ref else None,
            dpair.data_ptr() if with_pair else None, st), "ob_nbest_edit_distance")

    def mbr():
        _lib.check(lib.ob_mbr_select(
            dpair.data_ptr(), hyp.data_ptr(), hyp_len.data_ptr(), n_hyp.data_ptr(),
            score.data_ptr(), 1.0, B, N, T, out.data_ptr(), out_len.data_ptr(), best_k.data_ptr(),
            risk.data_ptr(), post.data_ptr(), st), "ob_mbr_select")

    def t(fn):
        return timed(fn, args.reps, args.warmup)

    res = {"edit_distance": t(lambda: pairs(False)),
           "edit_distance_ops": t(lambda: pairs(True)),
           "nbest_dpair": t(lambda: nbest(False, True)),
           "nbest_dref_ops": t(lambda: nbest(True, False)),
           "nbest_all": t(lambda: nbest(True, True)),
           "mbr_select_kernel": t(mbr),
           "mbr_select_python": t(lambda: mbr_select(hyp, hyp_len, n_hyp, score, 1.0)),
           "ctc_beam_search_nbest": t(lambda: ctc_beam_search_nbest_device(z, lens, N, None,
                                                                           BLANK))}
    torch.cuda.synchronize()
    live_pairs = int((n_hyp * (n_hyp - 1) // 2).sum().item())
    res.update(workspace_bytes=need, workspace_bytes_nbest=need_n, pairs_live=live_pairs,
               ref_len_mean=round(float(ref_len.float().mean().item()), 1),
               hyp_len_mean=round(float(best_len.float().mean().item()), 1),
               dist_mean=round(float(dist.float().mean().item()), 2),
               dpair_mean=round(float(dpair[dpair > 0].float().mean().item()), 2),
               mbr_pick_is_not_entry0=int((best_k != 0).sum().item()))

    # the host path: copy, then the Python double loop, one pair at a time
    def host_pairs():
        r, rl, h, hl = ref.cpu(), ref_len.cpu().tolist(), best.cpu(), best_len.cpu().tolist()
        return [levenshtein_distance(r[b, :rl[b]].tolist(), h[b, :hl[b]].tolist())
                for b in range(B)]

    assert host_pairs() == dist.cpu().tolist()
    res["host_levenshtein_pairs"] = host_clock(host_pairs, 3)
    U = min(args.host_utts, B)

    def host_pairwise():
        h, hl, nh = hyp[:U].cpu(), hyp_len[:U].cpu().tolist(), n_hyp[:U].cpu().tolist()
        d = []
        for b in range(U):
            e = [h[b, k, :hl[b][k]].tolist() for k in range(nh[b])]
            d.append([levenshtein_distance(e[j], e[k]) for j in range(nh[b])
                      for k in range(j + 1, nh[b])])
        return d

    got = host_pairwise()
    for b in range(U):
        n = int(n_hyp[b])
        want = [int(dpair[b, j, k]) for j in range(n) for k in range(j + 1, n)]
        assert got[b] == want, b
    hp = host_clock(host_pairwise, 1)
    n_host = sum(len(g) for g in got)
    res["host_levenshtein_pairwise"] = dict(hp, utterances=U, pairs=n_host,
                                            us_per_pair=round(hp["median_us"] / max(n_host, 1), 1),
                                            scaled_to_all_pairs_us=round(
                                                hp["median_us"] / max(n_host, 1) * live_pairs))

    fwd = {}
    if not args.skip_forward:
        from onebit_asr.conformer import ConformerASR
        from onebit_asr.data import CONFORMER_S, synthetic_batch

        torch.manual_seed(0)
        model = ConformerASR(80, V, **CONFORMER_S).to(dev).eval()
        batch = synthetic_batch([1000] * B, [40] * B, seed=1234, device=dev)
        batch["feat_lens"] = (lens * 4).clamp(max=1000).to(dev)
        with torch.no_grad():  # a blank bias that leaves about 15% of the frames to tokens
            _, _, lg = model(batch, precision=2)
            others = lg.clone()
            others[..., BLANK] = -float("inf")
            gap = (others.max(dim=-1).values - lg[..., BLANK]).flatten()
            model.ctc_head.bias[BLANK] += torch.quantile(gap[:1 << 20].float(), 0.85)
            del lg, others, gap
        plain = GraphedInference(model, precision=2, decoder="beam", beam_size=N)
        with_mbr = GraphedInference(model, precision=2, decoder="beam", beam_size=N, mbr_scale=1.0)
        plain.run(batch)
        with_mbr.run(batch)
        reps = max(3, args.reps // 2)
        a, b = [], []
        for _ in range(3):  # alternating, so that both see the same machine
            a.append(timed(lambda: plain.run(batch), reps, 1)["median_us"])
            b.append(timed(lambda: with_mbr.run(batch), reps, 1)["median_us"])
        torch.cuda.synchronize()
        hl = with_mbr.info["hyp_len"][:, 0].float()
        fwd = {"forward_beam_us": a, "forward_beam_mbr_us": b,
               "mbr_adds_us": round(statistics.median(b) - statistics.median(a), 1),
               "forward_hyp_len_mean_max": [round(float(hl.mean().item()), 1),
                                            int(hl.max().item())],
               "forward_mbr_pick_is_not_entry0": int((with_mbr.info["best_k"] != 0).sum().item())}
    line = json.dumps({"tool": "edit_bench", "device": torch.cuda.get_device_name(0), "B": B,
                       "T": T, "V": V, "nbest": N, "reps": args.reps, **res, **fwd,
                       "digest": _lib.source_digest()[:12]})
    print(line)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
