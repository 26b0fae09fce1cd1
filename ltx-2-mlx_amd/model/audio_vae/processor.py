"""Waveform -> the audio VAE encoder's input.  The reference stops short of this: its `load_audio_file` (pipelines/a2vid_two_stage.py:96-155)
returns a waveform and nothing turns that into the log-mel AudioEncoder reads.  AudioProcessor.waveform_to_mel does, with MelSTFT's two
convolutions (model/audio_vae/vocoder.py): the STFT is ltx2_audio_conv with a Hann-windowed DFT basis at stride = hop, the mel product a
1x1 conv whose operand staging takes the magnitude and whose epilogue is log(max(., 1e-5)).  Frames are centred (reflect padding by
n_fft / 2), the magnitude has power 1, the filterbank is the Slaney-scale, Slaney-normalised triangular one.

sample_rate 16000 / hop_length 160 / n_mels 64 are the reference's (AudioEncoder's defaults, A2VidConfig).  n_fft = win_length = 1024,
f_min = 0, f_max = 8000 are upstream's processor values to the best of the maintainers' knowledge and are NOT verified against released
weights; they are constructor arguments."""
from __future__ import annotations

import math
import os
import shutil
from typing import Optional, Tuple, Union

import numpy as np
import torch

from ... import _native as nv
from ... import kernels as K


def slaney_mel_filterbank(sample_rate: int, n_fft: int, n_mels: int, f_min: float, f_max: float) -> np.ndarray:
    """(n_mels, n_fft / 2 + 1) float64: triangles on the Slaney mel scale (linear below 1 kHz, log above: 200 / 3 Hz per mel, then
    ln(6.4) / 27 per mel), each scaled by 2 / (its band's width in Hz)."""
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0

    def hz_to_mel(f):
        f = np.asarray(f, dtype=np.float64)
        return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)

    def mel_to_hz(m):
        m = np.asarray(m, dtype=np.float64)
        return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)

    hz = mel_to_hz(np.linspace(hz_to_mel(f_min), hz_to_mel(f_max), n_mels + 2))
    freqs = np.linspace(0.0, sample_rate / 2.0, n_fft // 2 + 1)
    ramps = hz[:, None] - freqs[None, :]
    fdiff = np.diff(hz)
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    return np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (hz[2:] - hz[:-2]))[:, None]


def windowed_dft_basis(n_fft: int, win_length: int) -> np.ndarray:
    """(2 * (n_fft / 2 + 1), n_fft) float64: cos rows then -sin rows, times the periodic Hann window of win_length centred in n_fft."""
    n = np.arange(n_fft, dtype=np.float64)
    win = np.zeros(n_fft)
    left = (n_fft - win_length) // 2
    win[left:left + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)
    ang = 2.0 * np.pi * np.arange(n_fft // 2 + 1, dtype=np.float64)[:, None] * n[None, :] / n_fft
    return np.concatenate([np.cos(ang) * win, -np.sin(ang) * win])


class AudioProcessor:
    """waveform -> log-mel (1, 2, T_mel, n_mels) for AudioEncoder, on the GPU.  The bases are built on the host in float64 and cast to
    fp32 once."""

    def __init__(self, sample_rate: int = 16000, n_fft: int = 1024, win_length: int = 1024, hop_length: int = 160, n_mels: int = 64,
                 f_min: float = 0.0, f_max: float = 8000.0, device: Union[str, torch.device] = "cuda"):
        if win_length > n_fft or n_fft % 2:
            raise ValueError(f"AudioProcessor: win_length {win_length} must be <= n_fft {n_fft} (even)")
        self.sample_rate, self.n_fft, self.win_length, self.hop_length, self.n_mels = sample_rate, n_fft, win_length, hop_length, n_mels
        self.f_min, self.f_max = f_min, f_max
        self.n_freqs = n_fft // 2 + 1
        self.device = torch.device(device)
        self._packed = None

    def mel_frames(self, samples: int) -> int:
        """Centred frames of a waveform of `samples` samples (host only)."""
        return 1 + int(samples) // self.hop_length

    def samples_for_video(self, num_frames: int, fps: float) -> int:
        """Samples of num_frames / fps seconds (host only): what the waveform is cut or padded to before encoding."""
        return int(round(float(num_frames) / float(fps) * self.sample_rate))

    @staticmethod
    def fit_waveform(waveform: np.ndarray, samples: int) -> np.ndarray:
        """(C, n) -> (C, samples): cut, or right-pad with silence."""
        waveform = np.asarray(waveform)
        if waveform.shape[1] >= samples:
            return waveform[:, :samples]
        return np.concatenate([waveform, np.zeros((waveform.shape[0], samples - waveform.shape[1]), dtype=waveform.dtype)], axis=1)

    def _bases(self):
        if self._packed is None:
            stft = torch.from_numpy(windowed_dft_basis(self.n_fft, self.win_length).astype(np.float32))[:, None, :].to(self.device)
            mel = torch.from_numpy(slaney_mel_filterbank(self.sample_rate, self.n_fft, self.n_mels, self.f_min, self.f_max).astype(np.float32))
            self._packed = (K.pack_conv_weight(stft), K.pack_conv_weight(mel[:, :, None].to(self.device)))
        return self._packed

    def waveform_to_mel(self, waveform, sample_rate: int) -> torch.Tensor:
        """waveform [C, samples] (numpy or torch; C = 1 is duplicated to two channels) at self.sample_rate -> (1, 2, T_mel, n_mels) fp32
        with T_mel = 1 + samples // hop_length."""
        if self.device.type != "cuda":
            raise RuntimeError("AudioProcessor runs on the MI355X only (no CPU fallback): a CUDA processor")
        if int(sample_rate) != self.sample_rate:
            raise ValueError(f"AudioProcessor: waveform at {sample_rate} Hz, expected {self.sample_rate} (load_audio_file resamples)")
        w = torch.as_tensor(np.asarray(waveform) if not isinstance(waveform, torch.Tensor) else waveform).to(self.device, torch.float32)
        if w.dim() != 2 or w.shape[0] not in (1, 2):
            raise ValueError(f"AudioProcessor: waveform shape {tuple(w.shape)}, expected [1 or 2, samples]")
        half = self.n_fft // 2
        if w.shape[1] <= half:
            raise ValueError(f"AudioProcessor: {w.shape[1]} samples are too few to reflect-pad by n_fft / 2 = {half}")
        stft_w, mel_w = self._bases()
        frames = self.mel_frames(w.shape[1])
        padded = torch.cat([w[:, 1:half + 1].flip(1), w, w[:, -half - 1:-1].flip(1)], dim=1)          # reflect, the edge sample not repeated
        out = torch.empty(2, frames, self.n_mels, device=self.device)
        for c in range(w.shape[0]):
            spec = K.audio_conv1d(padded[c].contiguous()[:, None], stft_w, None, 2 * self.n_freqs, self.n_fft, stride=self.hop_length, t_out=frames)
            K.audio_conv1d(spec, mel_w, None, self.n_mels, 1, c_in=self.n_freqs, prologue=nv.AUDIO_PRO_MAGNITUDE, act=nv.AUDIO_ACT_LOG, out=out[c])
        if w.shape[0] == 1:
            out[1].copy_(out[0])
        return out[None]


def _read_wav(path: str) -> Tuple[np.ndarray, int]:
    """PCM .wav through the stdlib -> ((samples, channels) float32 in [-1, 1), rate); int16 / 32768 as the reference scales it."""
    import wave
    with wave.open(path, "rb") as wf:
        sr, n, ch, width = wf.getframerate(), wf.getnframes(), wf.getnchannels(), wf.getsampwidth()
        raw = wf.readframes(n)
    if width == 2:
        data = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif width == 4:
        data = (np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    elif width == 1:
        data = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    elif width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        data = ((v ^ 0x800000) - 0x800000).astype(np.float32) / 8388608.0
    else:
        raise ValueError(f"{path}: {8 * width}-bit PCM is not read")
    return data.reshape(-1, ch), sr


def load_audio_file(audio_path: str, target_sr: int = 16000, start_time: float = 0.0, max_duration: Optional[float] = None) -> Tuple[np.ndarray, int]:
    """Audio file -> (waveform [channels, samples] float32, sample rate), the reference's load_audio_file
    (pipelines/a2vid_two_stage.py:96-155) with its semantics: the start / duration trim at the file's rate, then the nearest-index
    resample to target_sr.  A .wav is read with the stdlib `wave`; anything else with `soundfile` when it imports, else through an
    `ffmpeg` on the path (to 16-bit stereo at target_sr, as the reference converts)."""
    if audio_path.lower().endswith(".wav"):
        data, sr = _read_wav(audio_path)
    else:
        try:
            import soundfile as sf
        except ImportError:
            sf = None
        if sf is not None:
            data, sr = sf.read(audio_path)
            data = np.asarray(data, dtype=np.float32)
        elif shutil.which("ffmpeg"):
            import subprocess
            import tempfile
            with tempfile.TemporaryDirectory() as tmp:
                wav = os.path.join(tmp, "a.wav")
                subprocess.run(["ffmpeg", "-v", "quiet", "-i", audio_path, "-ar", str(target_sr), "-ac", "2", "-y", wav], check=True)
                data, sr = _read_wav(wav)
        else:
            raise RuntimeError(f"{audio_path}: only .wav is read without the soundfile module or an ffmpeg binary")
    if data.ndim == 1:
        data = data[:, np.newaxis]
    if data.shape[0] > data.shape[1]:          # (samples, channels) -> (channels, samples), the reference's test
        data = data.T
    data = data[:, int(start_time * sr):]
    if max_duration is not None:
        data = data[:, :int(max_duration * sr)]
    if sr != target_sr:
        num_output = int(data.shape[1] * target_sr / sr)
        data = data[:, np.linspace(0, data.shape[1] - 1, num_output).astype(int)]
        sr = target_sr
    return np.ascontiguousarray(data), sr
