"""Feature front end on the device: Kaldi fbank + CMVN + SpecAugment + zero-padded collate for
a padded batch of 16 kHz waveforms (``ob_frontend_fwd``, csrc/frontend.hip), the part of the
reference that runs per utterance in DataLoader workers:

* src/data/dataset.py:117-135: ``torchaudio.compliance.kaldi.fbank(waveform, num_mel_bins=80,
  sample_frequency=16000)``, ``(fbank - mean) / std``, then SpecAugment on the train split;
* :150-209: SpecAugment (two frequency masks of width 27, two time masks of width 100);
* :245-273: the collate (features padded with 0.0, ``feat_lens``).

One launch, no host synchronisation, legal under HIP graph capture. The input is taken to be
16 kHz float32 at the amplitude the reference feeds torchaudio; resampling, int16 input, dither
and other Kaldi options are out of scope.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import _lib

__all__ = ["fbank_batch", "draw_specaug_starts", "FrontEnd", "fbank_num_frames", "frontend_table",
           "unpack_table"]

FRAME_LEN, N_FFT = 400, 512
MAX_MELS = 128
_TABLES: Dict[Tuple[str, int], torch.Tensor] = {}


def fbank_num_frames(n_samples: int) -> int:
    """Frames of an utterance of n_samples: 0 below 400, else 1 + (n - 400) // 160."""
    return int(_lib.load().ob_fbank_num_frames(int(n_samples)))


def frontend_table(n_mels: int = 80) -> torch.Tensor:
    """The kernel's constant table (window, twiddles, sparse mel bank; layout in
    include/onebit_hip.h) as a CPU float32 tensor, computed by the library on the host."""
    lib = _lib.load()
    n = lib.ob_frontend_table_floats(n_mels)
    if n <= 0:
        raise ValueError(f"n_mels must be in 1..{MAX_MELS}, got {n_mels}")
    t = torch.empty((n,), dtype=torch.float32)
    _lib.check(lib.ob_frontend_table_fill(t.data_ptr(), n_mels), "ob_frontend_table_fill")
    return t


def unpack_table(table: torch.Tensor, n_mels: int):
    """(window [400], twiddles [512, 2], dense mel bank [n_mels, 257]) of a table."""
    t = table.detach().cpu()
    window = t[:FRAME_LEN].clone()
    tw = t[FRAME_LEN:FRAME_LEN + 2 * N_FFT].reshape(N_FFT, 2).clone()
    desc = t[FRAME_LEN + 2 * N_FFT:FRAME_LEN + 2 * N_FFT + 3 * n_mels].reshape(n_mels, 3)
    wts = t[FRAME_LEN + 2 * N_FFT + 3 * n_mels:]
    bank = torch.zeros((n_mels, N_FFT // 2 + 1), dtype=torch.float32)
    for f in range(n_mels):
        first, count, off = (int(v) for v in desc[f])
        bank[f, first:first + count] = wts[off:off + count]
    return window, tw, bank


def _device_table(device: torch.device, n_mels: int) -> torch.Tensor:
    key = (str(device), n_mels)
    if key not in _TABLES:
        _TABLES[key] = frontend_table(n_mels).to(device)
    return _TABLES[key]


def _run(wave, wave_lens, table, n_mels, cmvn_mean, cmvn_std, starts, n_fmask, fmask_w, n_tmask,
         tmask_w, what):
    if not wave.is_cuda:
        raise RuntimeError(f"{what} runs on the HIP library (no CPU fallback)")
    if wave.dim() != 2:
        raise ValueError(f"wave must be [B, n_max], got {tuple(wave.shape)}")
    if wave.dtype != torch.float32:
        wave = wave.float()
    bsz, n_max = wave.shape
    if bsz > 0 and n_max > 0 and not (wave.stride(1) == 1 and wave.stride(0) >= n_max):
        wave = wave.contiguous()  # a row view with a larger stride is read in place
    stride = wave.stride(0) if bsz > 0 and n_max > 0 else n_max
    ln = wave_lens.to(device=wave.device, dtype=torch.int64).contiguous()
    if ln.shape != (bsz,):
        raise ValueError(f"wave_lens must be [{bsz}], got {tuple(ln.shape)}")
    lib = _lib.load()
    n_frames = lib.ob_fbank_num_frames(n_max)
    feats = torch.empty((bsz, n_frames, n_mels), dtype=torch.float32, device=wave.device)
    feat_lens = torch.empty((bsz,), dtype=torch.int64, device=wave.device)
    if starts is not None:
        starts = starts.to(device=wave.device, dtype=torch.int32).contiguous()
        if starts.shape != (bsz, n_fmask + n_tmask):
            raise ValueError(f"starts must be [{bsz}, {n_fmask + n_tmask}], got "
                             f"{tuple(starts.shape)}")
    _lib.check(lib.ob_frontend_fwd(wave.data_ptr(), stride, ln.data_ptr(), bsz, n_max,
                                   table.data_ptr(), n_mels, _lib.ptr(cmvn_mean),
                                   _lib.ptr(cmvn_std), _lib.ptr(starts), n_fmask, fmask_w,
                                   n_tmask, tmask_w, feats.data_ptr(), n_frames,
                                   feat_lens.data_ptr(), _lib.stream_of(wave)), "ob_frontend_fwd")
    return feats, feat_lens


def fbank_batch(wave: torch.Tensor, wave_lens: torch.Tensor, n_mels: int = 80
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """wave [B, n_max] fp32 (device, 16 kHz), wave_lens [B] samples -> (feats fp32
    [B, T, n_mels] with T = fbank_num_frames(n_max), rows past an utterance's frames 0.0;
    feat_lens int64 [B]). Plain Kaldi log-mel filterbank, no CMVN, no masks."""
    if not wave.is_cuda:
        raise RuntimeError("fbank_batch runs on the HIP library (no CPU fallback)")
    if not 1 <= n_mels <= MAX_MELS:
        raise ValueError(f"n_mels must be in 1..{MAX_MELS}, got {n_mels}")
    return _run(wave, wave_lens, _device_table(wave.device, n_mels), n_mels, None, None, None,
                0, 0, 0, 0, "fbank_batch")


def draw_specaug_starts(feat_lens: torch.Tensor, generator: Optional[torch.Generator] = None,
                        freq_mask_param: int = 27, time_mask_param: int = 100,
                        num_freq_mask: int = 2, num_time_mask: int = 2, n_mels: int = 80
                        ) -> torch.Tensor:
    """Mask starts for ``FrontEnd``: int32 [B, num_freq_mask + num_time_mask], frequency masks
    first. As dataset.py:194-207 every mask has the fixed width min(param, size) and its start
    is uniform in [0, max(1, size - width)): size is n_mels for a frequency mask and the
    utterance's own frame count for a time mask. Computed as floor(rand * range) on the device
    of ``feat_lens`` (a device tensor stays on the device: no host synchronisation);
    ``generator`` may live on that device or on the CPU."""
    dev = feat_lens.device
    bsz = feat_lens.shape[0]
    gdev = generator.device if generator is not None else dev
    u = torch.rand((bsz, num_freq_mask + num_time_mask), generator=generator, device=gdev,
                   dtype=torch.float64).to(dev)
    m = feat_lens.to(torch.int64)
    range_t = (m - m.clamp(max=time_mask_param)).clamp(min=1)
    range_f = max(1, n_mels - min(freq_mask_param, n_mels))
    rng = torch.cat([torch.full((bsz, num_freq_mask), range_f, dtype=torch.int64, device=dev),
                     range_t[:, None].expand(bsz, num_time_mask)], dim=1)
    starts = torch.minimum(torch.floor(u * rng).to(torch.int64), rng - 1)
    return starts.to(torch.int32)


class FrontEnd(torch.nn.Module):
    """Waveforms to the batch dict's ``feats`` / ``feat_lens`` on the device.

    ``cmvn_mean`` / ``cmvn_std``: [n_mels] statistics, or pass the reference's ``cmvn_stats``
    dict (``{"mean": ..., "std": ...}``, dataset.py:130) as ``cmvn_mean``. ``spec_augment``:
    None, or a dict with the reference's SpecAugment arguments (``freq_mask_param``,
    ``time_mask_param``, ``num_freq_mask``, ``num_time_mask``; ``{}`` for its defaults 27, 100,
    2, 2). The masks are applied in ``.training`` mode only, as the reference applies them to the
    train split only; if no ``starts`` are given there, they are drawn
    (``draw_specaug_starts``, from ``generator`` when one was passed to the constructor).

    As in the reference the masks have a fixed width, so an utterance of at most
    ``time_mask_param`` frames is zeroed entirely by its time mask.
    """

    def __init__(self, cmvn_mean=None, cmvn_std=None, spec_augment: Optional[dict] = None,
                 n_mels: int = 80, generator: Optional[torch.Generator] = None):
        super().__init__()
        if not 1 <= n_mels <= MAX_MELS:
            raise ValueError(f"n_mels must be in 1..{MAX_MELS}, got {n_mels}")
        if isinstance(cmvn_mean, dict):
            if cmvn_std is not None:
                raise ValueError("pass either a cmvn_stats dict or cmvn_mean and cmvn_std")
            cmvn_mean, cmvn_std = cmvn_mean["mean"], cmvn_mean["std"]
        if (cmvn_mean is None) != (cmvn_std is None):
            raise ValueError("cmvn_mean and cmvn_std go together")
        self.n_mels = n_mels
        self.register_buffer("table", frontend_table(n_mels), persistent=False)
        if cmvn_mean is not None:
            mean = torch.as_tensor(cmvn_mean, dtype=torch.float32).reshape(-1).clone()
            std = torch.as_tensor(cmvn_std, dtype=torch.float32).reshape(-1).clone()
            if mean.numel() != n_mels or std.numel() != n_mels:
                raise ValueError(f"CMVN statistics must have {n_mels} elements")
        else:
            mean = std = None
        self.register_buffer("cmvn_mean", mean)
        self.register_buffer("cmvn_std", std)
        sa = {"freq_mask_param": 27, "time_mask_param": 100, "num_freq_mask": 2,
              "num_time_mask": 2}
        if spec_augment is not None:
            unknown = set(spec_augment) - set(sa)
            if unknown:
                raise ValueError(f"unknown spec_augment keys {sorted(unknown)}")
            sa.update(spec_augment)
        self.spec_augment = sa if spec_augment is not None else None
        self.generator = generator

    def forward(self, wave: torch.Tensor, wave_lens: torch.Tensor,
                starts: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        if not wave.is_cuda:
            raise RuntimeError("FrontEnd runs on the HIP library (no CPU fallback)")
        if self.table.device != wave.device:
            raise RuntimeError(f"FrontEnd is on {self.table.device}, wave on {wave.device}")
        sa = self.spec_augment if self.training else None
        if sa is None:
            feats, lens = _run(wave, wave_lens, self.table, self.n_mels, self.cmvn_mean,
                               self.cmvn_std, None, 0, 0, 0, 0, "FrontEnd")
            return {"feats": feats, "feat_lens": lens}
        if starts is None:
            n_max = wave.shape[1]
            m = wave_lens.to(device=wave.device, dtype=torch.int64).clamp(min=0, max=n_max)
            m = torch.where(m < FRAME_LEN, torch.zeros_like(m), 1 + (m - FRAME_LEN) // 160)
            starts = draw_specaug_starts(m, self.generator, n_mels=self.n_mels, **sa)
        feats, lens = _run(wave, wave_lens, self.table, self.n_mels, self.cmvn_mean,
                           self.cmvn_std, starts, sa["num_freq_mask"], sa["freq_mask_param"],
                           sa["num_time_mask"], sa["time_mask_param"], "FrontEnd")
        return {"feats": feats, "feat_lens": lens}
