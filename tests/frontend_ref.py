"""Test helper (not a test): the feature front end that ``ob_frontend_fwd`` documents
(include/onebit_hip.h), restated in numpy fp64 step by step. It is the arithmetic definition of
``torchaudio.compliance.kaldi.fbank(waveform, num_mel_bins=80, sample_frequency=16000)`` with its
defaults (src/data/dataset.py:124-128), the CMVN of :130-131, the SpecAugment of :150-209 with
the mask starts as an input, and the zero-padded collate of :245-273; not an optimised form.

``fbank_ref32`` is the same steps in torch fp32 with ``torch.fft.rfft``: the arithmetic the
reference's torchaudio call performs on the host.

Steps for an utterance of n samples:
  frames   m = 0 if n < 400 else 1 + (n - 400) // 160; frame i = samples [160 i, 160 i + 400)
  DC       subtract the frame's own mean
  preemph  y[j] = x[j] - 0.97 x[max(j - 1, 0)]
  window   w[j] = (0.5 - 0.5 cos(2 pi j / 399)) ** 0.85, zero-pad to 512
  power    P[k] = |rfft_512(y)[k]|^2, k = 0..256
  mel      E[f] = sum_k bank[f][k] P[k]
  log      log(max(E, 1.1920929e-07))
  CMVN     (v - mean) / std
  masks    fixed width min(param, size), start given; masked elements are 0.0
  collate  rows m..T-1 are 0.0
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np

FRAME_LEN, FRAME_SHIFT, N_FFT = 400, 160, 512
SAMPLE_RATE, LOW_FREQ, HIGH_FREQ = 16000.0, 20.0, 8000.0
PREEMPH = 0.97
LOG_FLOOR = float(np.float32(1.1920929e-07))


def num_frames(n: int) -> int:
    return 0 if n < FRAME_LEN else 1 + (n - FRAME_LEN) // FRAME_SHIFT


def mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def povey_window() -> np.ndarray:
    j = np.arange(FRAME_LEN, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * math.pi * j / (FRAME_LEN - 1))) ** 0.85


def twiddles() -> np.ndarray:
    """(cos, -sin)(2 pi t / 512), t = 0..511: exp(-2 pi i t / 512) as [512, 2]."""
    t = np.arange(N_FFT, dtype=np.float64)
    return np.stack([np.cos(2.0 * math.pi * t / N_FFT), -np.sin(2.0 * math.pi * t / N_FFT)], 1)


def mel_bank(n_mels: int = 80) -> np.ndarray:
    """[n_mels, 257] triangular weights, linear in mel between mel(20) and mel(8000)."""
    lo, hi = float(mel(LOW_FREQ)), float(mel(HIGH_FREQ))
    d = (hi - lo) / (n_mels + 1)
    bank = np.zeros((n_mels, N_FFT // 2 + 1), dtype=np.float64)
    mk = mel(np.arange(N_FFT // 2) * (SAMPLE_RATE / N_FFT))
    for f in range(n_mels):
        left, centre, right = lo + f * d, lo + (f + 1) * d, lo + (f + 2) * d
        up = (mk - left) / (centre - left)
        down = (right - mk) / (right - centre)
        bank[f, :N_FFT // 2] = np.maximum(0.0, np.minimum(up, down))
    return bank  # bin 256 stays 0


def frames_of(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    m = num_frames(len(x))
    idx = FRAME_SHIFT * np.arange(m)[:, None] + np.arange(FRAME_LEN)[None, :]
    return x[idx] if m else np.zeros((0, FRAME_LEN))


def remove_dc(fr: np.ndarray) -> np.ndarray:
    return fr - fr.mean(axis=1, keepdims=True)


def preemphasis(fr: np.ndarray) -> np.ndarray:
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)  # x[max(j - 1, 0)]
    return fr - PREEMPH * prev


def windowed_frames(x: np.ndarray) -> np.ndarray:
    return preemphasis(remove_dc(frames_of(x))) * povey_window()[None, :]


def power_spectrum(y: np.ndarray) -> np.ndarray:
    """y [m, 400] windowed frames -> [m, 257]."""
    pad = np.zeros((y.shape[0], N_FFT), dtype=np.float64)
    pad[:, :FRAME_LEN] = y
    s = np.fft.rfft(pad, axis=1)
    return s.real ** 2 + s.imag ** 2


def fbank(x: np.ndarray, n_mels: int = 80) -> np.ndarray:
    """One utterance, fp64: [m, n_mels]."""
    p = power_spectrum(windowed_frames(x))
    return np.log(np.maximum(p @ mel_bank(n_mels).T, LOG_FLOOR))


def spec_augment(v: np.ndarray, starts: Sequence[int], n_fmask: int, fmask_w: int, n_tmask: int,
                 tmask_w: int) -> np.ndarray:
    """dataset.py:184-209 with the starts given: frequency masks first, then time masks."""
    v = v.copy()
    m, nb = v.shape
    wf, wt = min(fmask_w, nb), min(tmask_w, m)
    for s in starts[:n_fmask]:
        v[:, s:s + wf] = 0.0
    for s in starts[n_fmask:n_fmask + n_tmask]:
        v[s:s + wt, :] = 0.0
    return v


def start_range(size: int, width_param: int) -> int:
    """torch.randint(0, max(1, size - min(param, size))): the exclusive upper bound."""
    return max(1, size - min(width_param, size))


def frontend(wave: np.ndarray, wave_lens: Sequence[int], n_mels: int = 80, T: Optional[int] = None,
             cmvn_mean=None, cmvn_std=None, starts=None, n_fmask: int = 2, fmask_w: int = 27,
             n_tmask: int = 2, tmask_w: int = 100):
    """Padded batch: wave [B, n_max] -> (feats fp64 [B, T, n_mels], feat_lens int64 [B])."""
    bsz, n_max = wave.shape
    T = num_frames(n_max) if T is None else T
    feats = np.zeros((bsz, T, n_mels), dtype=np.float64)
    lens = np.zeros((bsz,), dtype=np.int64)
    for b in range(bsz):
        n = int(min(max(int(wave_lens[b]), 0), n_max))
        v = fbank(wave[b, :n], n_mels)
        if cmvn_mean is not None:
            v = (v - np.asarray(cmvn_mean, np.float64)) / np.asarray(cmvn_std, np.float64)
        if starts is not None:
            v = spec_augment(v, [int(s) for s in starts[b]], n_fmask, fmask_w, n_tmask, tmask_w)
        feats[b, :v.shape[0]] = v
        lens[b] = v.shape[0]
    return feats, lens


def fbank_ref32(x, n_mels: int = 80):
    """One utterance in torch fp32 with torch.fft.rfft: what the reference's host call computes.
    x: 1-D float tensor or array; returns a float32 tensor [m, n_mels]."""
    import torch

    x = torch.as_tensor(x, dtype=torch.float32)
    m = num_frames(x.numel())
    if m == 0:
        return torch.zeros((0, n_mels), dtype=torch.float32)
    fr = x.unfold(0, FRAME_LEN, FRAME_SHIFT)[:m]
    fr = fr - fr.mean(dim=1, keepdim=True)
    prev = torch.cat([fr[:, :1], fr[:, :-1]], dim=1)
    fr = fr - PREEMPH * prev
    j = torch.arange(FRAME_LEN, dtype=torch.float32)
    win = (0.5 - 0.5 * torch.cos(2.0 * math.pi * j / (FRAME_LEN - 1))).pow(0.85)
    fr = torch.nn.functional.pad(fr * win, (0, N_FFT - FRAME_LEN))
    spec = torch.fft.rfft(fr, dim=1)
    power = spec.real ** 2 + spec.imag ** 2
    bank = torch.from_numpy(mel_bank(n_mels)).to(torch.float32)
    e = power @ bank.T
    return torch.log(torch.clamp(e, min=LOG_FLOOR))


def make_wave(lens: Sequence[int], n_max: int, seed: int = 0) -> np.ndarray:
    """Uniform noise of amplitude 0.1 plus two tones per utterance (so that no mel energy is near
    the log floor), float32 [B, n_max]; samples past an utterance's length are filled too (the
    front end must not read them into its result)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n_max, dtype=np.float64) / SAMPLE_RATE
    out = np.empty((len(lens), n_max), dtype=np.float32)
    for b in range(len(lens)):
        f1, f2 = 220.0 * (b + 1), 3100.0 + 157.0 * b
        x = rng.uniform(-0.1, 0.1, n_max) + 0.05 * np.sin(2 * math.pi * f1 * t) \
            + 0.03 * np.sin(2 * math.pi * f2 * t + 0.5)
        out[b] = x.astype(np.float32)
    return out

