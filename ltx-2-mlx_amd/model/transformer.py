"""LTX-2 DiT behind the reference's model API: Modality, LTXModel, X0Model.

Mirrors (names, argument meaning, error behaviour) reference
LTX_2_MLX/model/transformer/model.py:59-69 (Modality), :413-881 (LTXModel), :884-936 (X0Model)
for the VideoOnly and AudioVideo models (19B blocks and the V2.3 variant).  All arithmetic runs in libltx2hip.so (ltx2_dit_* engine calls);
torch owns device memory and streams only.  Step-invariant per-prompt work (caption projection,
cross-attention K/V, RoPE tables) is computed once per (context, positions) pair in
``prepare`` -- the reference recomputes it every step (model.py:262-271) with identical results.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from dataclasses import dataclass
from enum import Enum
from typing import Dict, List, Optional, Sequence, Tuple, Union

import re

import torch

from .. import _native as nv
from .. import kernels as K

BF16 = torch.bfloat16


class LTXModelType(Enum):
    AudioVideo = "ltx av model"
    VideoOnly = "ltx video only model"
    AudioOnly = "ltx audio only model"

    def is_video_enabled(self) -> bool:
        return self in (LTXModelType.AudioVideo, LTXModelType.VideoOnly)

    def is_audio_enabled(self) -> bool:
        return self in (LTXModelType.AudioVideo, LTXModelType.AudioOnly)


class LTXRopeType(Enum):
    INTERLEAVED = "interleaved"
    SPLIT = "split"



class Fp8Weight:
    """A linear weight kept as float8_e4m3fn codes + the checkpoint's per-tensor `weight_scale` (reference loader/fp8_loader.py:14-51
    dequantises it at load: f32(code) * scale -> compute dtype).  Passed through load_state_dict it stays fp8 in HBM and the GEMM
    expands it on the fly with the same arithmetic."""

    def __init__(self, codes: torch.Tensor, scale: float):
        if codes.element_size() != 1 or codes.dim() != 2:
            raise ValueError("Fp8Weight: codes must be a 2-D float8_e4m3fn (or uint8 view) tensor")
        self.codes, self.scale = codes, float(scale)

    @property
    def shape(self):
        return self.codes.shape


FP8_RESIDENT_KEYS = re.compile(r"^transformer_blocks\.\d+\.(attn1|attn2)\.(to_q|to_k|to_v|to_out\.0)\.weight$|^transformer_blocks\.\d+\.ff\.net\.(0\.proj|2)\.weight$")


@dataclass
class Modality:
    """Input record (reference model.py:59-69)."""
    latent: torch.Tensor                  # (B, T, C) patchified latents
    context: torch.Tensor                 # (B, S, C_ctx) text context
    context_mask: Optional[torch.Tensor]  # boolean / 0-1 integer key mask (B, S), True = attend; None on every live path (pipelines/common.py:223-232)
    timesteps: torch.Tensor               # (B,) or (B, T) / (B, T, 1)
    positions: torch.Tensor               # (B, 3, T, 2) [start, end) in (seconds, px, px)
    enabled: bool = True
    sigma: Optional[torch.Tensor] = None


def rope_tables_token_major(positions: torch.Tensor, dim: int, heads: int, theta: float,
                            max_pos: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """SPLIT RoPE cos/sin, fp32, token-major [N, dim/2] with slot h*(d/2)+j for head h.

    Host-side per-prompt setup restating precompute_freqs_cis(SPLIT, use_middle_indices_grid=True)
    (reference model/transformer/rope.py:181-211,242-328,365-418): freq grid
    theta**linspace(0,1,dim//(2*n_dims)) * pi/2, fractional mid positions scaled to [-1,1], slot
    order f*n_dims + d, identity padding at the FRONT.  CPU fp32 restatement kept for host-side tests; the
    model builds its tables on the GPU with `kernels.rope_tables` (ltx2_rope_tables), same formula."""
    pos = positions.detach().float().cpu()
    assert pos.shape[0] == 1, "batch is 1"
    n_dims = pos.shape[1]
    if n_dims != len(max_pos):
        raise ValueError(f"Number of position dimensions ({n_dims}) must match max_pos length ({len(max_pos)})")
    n_freq = dim // (2 * n_dims)
    grid = (torch.tensor(float(theta)) ** torch.linspace(0.0, 1.0, n_freq, dtype=torch.float32) * (math.pi / 2)).float()
    mid = (pos[0, :, :, 0] + pos[0, :, :, 1]) / 2.0                       # [n_dims, N]
    frac = torch.stack([mid[i] / max_pos[i] for i in range(n_dims)], dim=-1)   # [N, n_dims]
    freqs = grid[None, None, :] * (frac * 2 - 1)[:, :, None]                # [N, n_dims, n_freq]
    freqs = freqs.transpose(1, 2).reshape(freqs.shape[0], -1)               # slot = f*n_dims + d
    cos, sin = torch.cos(freqs), torch.sin(freqs)
    pad = dim // 2 - freqs.shape[-1]
    if pad:
        cos = torch.cat([torch.ones(cos.shape[0], pad), cos], dim=-1)
        sin = torch.cat([torch.zeros(sin.shape[0], pad), sin], dim=-1)
    return cos.contiguous(), sin.contiguous()


class LTXModel:
    """Velocity model.  Constructor keywords follow reference model.py:436-461; VideoOnly and
    AudioVideo model types, 19B-style blocks or V2.3 (cross_attention_adaln / apply_gated_attention)."""

    AUDIO_ATTENTION_HEADS = 32          # reference model.py:428-434
    AUDIO_HEAD_DIM = 64
    AUDIO_IN_CHANNELS = 128
    AUDIO_OUT_CHANNELS = 128
    AUDIO_CROSS_PE_MAX_POS = 20

    def __init__(self, model_type: LTXModelType = LTXModelType.VideoOnly, num_attention_heads: int = 32,
                 attention_head_dim: int = 128, in_channels: int = 128, out_channels: int = 128, num_layers: int = 48,
                 cross_attention_dim: int = 4096, norm_eps: float = 1e-6, caption_channels: Optional[int] = 3840,
                 positional_embedding_theta: float = 10000.0, positional_embedding_max_pos: Optional[List[int]] = None,
                 timestep_scale_multiplier: int = 1000, av_ca_timestep_scale_multiplier: int = 1,
                 use_middle_indices_grid: bool = True, rope_type: LTXRopeType = LTXRopeType.SPLIT,
                 compute_dtype: torch.dtype = BF16, low_memory: bool = False, fast_mode: bool = False,
                 cross_attention_adaln: bool = False, apply_gated_attention: bool = False,
                 device: Union[str, torch.device] = "cuda", audio_attention_heads: Optional[int] = None, fp8_compute: bool = False):
        if model_type == LTXModelType.AudioOnly:
            raise NotImplementedError("AudioOnly transformer is outside the denoise hot path (DESIGN.md)")
        if rope_type != LTXRopeType.SPLIT or not use_middle_indices_grid:
            raise NotImplementedError("the DiT uses SPLIT RoPE with middle-of-bounds positions (model.py:455,453)")
        if compute_dtype not in (BF16, torch.float16):
            raise NotImplementedError("compute dtype is bfloat16 or float16 operands (fp32 accumulate / residual stream); fp32 operands are not built")
        self._L = nv.lib(compute_dtype)        # bfloat16 -> libltx2hip.so, float16 (the reference's default) -> libltx2hip_f16.so
        self.model_type = model_type
        self.is_av = model_type == LTXModelType.AudioVideo
        self.num_attention_heads = num_attention_heads
        self.attention_head_dim = attention_head_dim
        self.inner_dim = self.video_inner_dim = num_attention_heads * attention_head_dim
        self.audio_heads = audio_attention_heads or self.AUDIO_ATTENTION_HEADS
        self.audio_inner_dim = self.audio_heads * self.AUDIO_HEAD_DIM
        self.in_channels, self.out_channels, self.num_layers = in_channels, out_channels, num_layers
        self.caption_channels = caption_channels
        self.norm_eps = norm_eps
        self.positional_embedding_theta = positional_embedding_theta
        self.positional_embedding_max_pos = positional_embedding_max_pos or [20, 2048, 2048]
        self.timestep_scale_multiplier = timestep_scale_multiplier
        self.av_ca_timestep_scale_multiplier = av_ca_timestep_scale_multiplier
        self.cross_attention_adaln = cross_attention_adaln
        self.apply_gated_attention = apply_gated_attention
        self.compute_dtype = compute_dtype
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("LTXModel runs on the MI355X only (no CPU fallback); got device " + str(device))
        if self.is_av and self.audio_heads != num_attention_heads:
            raise ValueError("AudioVideo: audio heads must equal video heads (shared cross-modal RoPE head split, model.py:336-343)")
        cfg = nv.DitConfig(num_layers, num_attention_heads, attention_head_dim, in_channels, out_channels,
                           caption_channels or 0, norm_eps, float(timestep_scale_multiplier),
                           nv.MODEL_AUDIO_VIDEO if self.is_av else nv.MODEL_VIDEO_ONLY, self.audio_heads, self.AUDIO_HEAD_DIM,
                           self.AUDIO_IN_CHANNELS, self.AUDIO_OUT_CHANNELS, int(cross_attention_adaln),
                           int(apply_gated_attention), float(av_ca_timestep_scale_multiplier))
        h = C.c_void_p()
        nv.check(self._L.ltx2_dit_create(C.byref(cfg), C.byref(h)))
        self._h = h
        # MI355X addition (BASELINE config 3, "fp8 weights (CDNA4 fp8 MFMA)"): opt-in fp8 COMPUTE.  The video stream's attention /
        # feed-forward projections keep e4m3fn weights (an fp8 checkpoint's codes, or bf16 weights quantised per output channel at
        # load), their activations are quantised per token inside the step, and the products run on the fp8 MFMA at twice the bf16
        # rate.  Not the parity-exact default: the reference dequantises fp8 checkpoints at load (loader/fp8_loader.py:54-130).
        self.fp8_compute = bool(fp8_compute)
        if self.fp8_compute:
            nv.check(self._L.ltx2_dit_set_option(h, b"fp8_compute", 1))
        self._w: Dict[str, torch.Tensor] = {}
        self._ws: Optional[torch.Tensor] = None
        self._bound: Tuple[int, ...] = (0, 0, 0, 0, 0)
        self._prep_key = None
        self._mask_refs = {}
        self._prep_refs = None
        self._clone: Optional["LTXModel"] = None       # clone_sharing_weights()
        self._twin: Optional["LTXModel"] = None        # VideoOnly engine over the SAME weight tensors (video-only inference on an AV model)
        self._sigma_dev: Dict[float, torch.Tensor] = {}  # device scalars of the step sigmas (no host-to-device copy inside the loop)
        self._stg: Dict[int, Optional[bytes]] = {0: None, 1: None}     # per modality, the engine's STG skip flags (set_stg_blocks); None: no set
        self._xattn: Tuple[float, int] = (1.0, 0)                      # set_cross_attn_scale: (scale, start_layer); a clone is given the same
        self._graph_owner: Optional[Tuple[str, "LTXModel"]] = None     # (kind of the last capture made through this object, the context that holds its graph)
        self._ctor = dict(num_attention_heads=num_attention_heads, attention_head_dim=attention_head_dim, in_channels=in_channels,
                          out_channels=out_channels, num_layers=num_layers, cross_attention_dim=cross_attention_dim, norm_eps=norm_eps,
                          caption_channels=caption_channels, positional_embedding_theta=positional_embedding_theta,
                          positional_embedding_max_pos=positional_embedding_max_pos, timestep_scale_multiplier=timestep_scale_multiplier,
                          cross_attention_adaln=cross_attention_adaln, apply_gated_attention=apply_gated_attention, device=device,
                          fp8_compute=fp8_compute, compute_dtype=compute_dtype)

    def set_option(self, name: str, value: int) -> None:
        """Engine option by name (ltx2_dit_set_option; include/ltx2hip.h lists them)."""
        nv.check(self._L.ltx2_dit_set_option(self._h, name.encode(), int(value)))

    def _video_twin(self) -> "LTXModel":
        """The video half of this AudioVideo model as a VideoOnly engine: with no audio tokens the reference's blocks run only
        video self-attention, text cross-attention and the video feed-forward (transformer.py:479-483: run_ax and run_a2v are
        False for an empty audio stream), which is exactly the VideoOnly program over the video weights.  No weight is copied."""
        if self._twin is None:
            t = LTXModel(model_type=LTXModelType.VideoOnly, **self._ctor)
            for k, v in self._w.items():
                t._register(k, v)
            t._put_stg_flags(0, self._stg[0])
            self._twin = t
        return self._twin

    # ------------------------------------------------------------------ STG: the self-attentions a perturbed forward skips
    def _set_ctx_flags(self, modality: int, flags: Optional[bytes]) -> None:
        """This context's set alone (self._stg mirrors what the engine holds)."""
        if self._stg[modality] != flags:
            nv.check(self._L.ltx2_dit_set_stg_blocks(self._h, modality, flags, 0 if flags is None else len(flags)))
            self._stg[modality] = flags

    def _put_stg_flags(self, modality: int, flags: Optional[bytes]) -> None:
        self._set_ctx_flags(modality, flags)
        if modality == 0 and self._twin is not None:
            self._twin._put_stg_flags(0, flags)

    @contextlib.contextmanager
    def _stg_override(self, flags: Tuple[Optional[bytes], Optional[bytes]]):
        """The sets of one __call__(..., perturbations=...) on this context, for the duration of the call: the engine reads them while it
        enqueues, so the sets of set_stg_blocks are put back as soon as the call returns."""
        prev = dict(self._stg)
        try:
            for k in ((0, 1) if self.is_av else (0,)):
                self._set_ctx_flags(k, flags[k])
            yield
        finally:
            for k, f in prev.items():
                self._set_ctx_flags(k, f)

    def set_stg_blocks(self, blocks: Optional[Sequence[int]], modality: int = 0) -> None:
        """The layers whose self-attention the perturbed forward (__call__(..., perturbations=...), stg_step_, the captured STG loop) skips:
        modality 0 video, 1 audio (AudioVideo models).  None: every layer; an empty list clears the set.  An AudioVideo model hands the video
        set on to its video twin.  The plain forward and every other step ignore it (ltx2_dit_set_stg_blocks)."""
        if modality not in (0, 1) or (modality == 1 and not self.is_av):
            raise ValueError(f"modality={modality}: 0 (video), or 1 (audio) on an AudioVideo model")
        idx = list(range(self.num_layers)) if blocks is None else [int(b) for b in blocks]
        bad = [b for b in idx if not 0 <= b < self.num_layers]
        if bad:
            raise ValueError(f"stg_blocks {bad} out of range: the model has {self.num_layers} layers")
        flags = bytearray(self.num_layers)
        for b in idx:
            flags[b] = 1
        self._put_stg_flags(modality, bytes(flags) if idx else None)

    def _perturbation_flags(self, perturbations) -> Optional[Tuple[Optional[bytes], Optional[bytes]]]:
        """A BatchedPerturbationConfig of batch 1 -> (video flags, audio flags) for ltx2_dit_set_stg_blocks; None: nothing is perturbed."""
        from ..components.perturbations import BatchedPerturbationConfig, PerturbationType as PT
        if perturbations is None:
            return None
        if not isinstance(perturbations, BatchedPerturbationConfig):
            raise TypeError("perturbations must be a BatchedPerturbationConfig")
        if len(perturbations.perturbations) != 1:
            raise ValueError("batch must be 1 (one PerturbationConfig)")
        L = range(self.num_layers)
        for kind in (PT.SKIP_A2V_CROSS_ATTN, PT.SKIP_V2A_CROSS_ATTN):
            if any(perturbations.any_in_batch(kind, l) for l in L):
                raise NotImplementedError(f"{kind.name}: the cross-modal perturbations are not built (they would cut into the AudioVideo stream schedule)")
        out = []
        for kind in (PT.SKIP_VIDEO_SELF_ATTN, PT.SKIP_AUDIO_SELF_ATTN):
            f = bytes(1 if perturbations.all_in_batch(kind, l) else 0 for l in L)
            out.append(f if any(f) else None)
        return None if out == [None, None] else (out[0], out[1])

    def clone_sharing_weights(self) -> "LTXModel":
        """A second engine context of the SAME model over the SAME weight tensors (nothing is copied): its own workspace and per-prompt
        setup.  The guided loops evaluate the negative prompt through it, so neither context re-projects its text K / V every step."""
        if self._clone is None:
            extra = dict(av_ca_timestep_scale_multiplier=self.av_ca_timestep_scale_multiplier, audio_attention_heads=self.audio_heads) if self.is_av else {}
            t = LTXModel(model_type=self.model_type, **self._ctor, **extra)
            for k, v in self._w.items():
                t._register(k, v)
            if self._xattn[0] != 1.0:
                t.set_cross_attn_scale(*self._xattn)
            self._clone = t
        return self._clone

    def set_cross_attn_scale(self, scale: float, start_layer: int = 40) -> None:
        """The reference's LTXModel.set_cross_attn_scale: from now on the text cross-attention output of the layers >= start_layer is multiplied by
        `scale` before it joins the residual stream (ltx2_dit_set_cross_attn_scale: a gate table of the out-projection's epilogue, no further
        kernel); 1.0 removes it.  The context of clone_sharing_weights() follows.  NotImplementedError on an AudioVideo model and on a gated
        text cross-attention (LTX-2.3): their gate is per row."""
        nv.check(self._L.ltx2_dit_set_cross_attn_scale(self._h, float(scale), int(start_layer)))
        self._xattn = (float(scale), int(start_layer))
        if self._clone is not None:
            self._clone.set_cross_attn_scale(scale, start_layer)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                if getattr(self, "_fbc", (0.0, 0))[1]:          # the first-block cache's buffers live beside the context: freed before it
                    self._L.ltx2_dit_fbc_configure(self._h, 0, 0.0)
                self._L.ltx2_dit_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def _attn_specs(self) -> List[Tuple[str, int, int, int, int, bool]]:
        """(block-relative name, query dim, context dim, inner dim, heads, is_self) per attention module
        (transformer.py:283-365)."""
        dv, da, hv, ha = self.inner_dim, self.audio_inner_dim, self.num_attention_heads, self.audio_heads
        a = [("attn1", dv, dv, dv, hv, True), ("attn2", dv, dv, dv, hv, False)]
        if self.is_av:
            a += [("audio_attn1", da, da, da, ha, True), ("audio_attn2", da, da, da, ha, False),
                  ("audio_to_video_attn", dv, da, da, ha, False), ("video_to_audio_attn", da, dv, da, ha, False)]
        return a

    def expected_weight_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """Checkpoint keys (after stripping 'model.diffusion_model.', reference
        loader/weight_converter.py:277-315) and shapes this model consumes."""
        dv, da = self.inner_dim, self.audio_inner_dim
        rows = 9 if self.cross_attention_adaln else 6
        s: Dict[str, Tuple[int, ...]] = {}

        def lin(n, o, i):
            s[n + ".weight"] = (o, i)
            s[n + ".bias"] = (o,)

        def adaln(n, d, r):
            lin(n + ".emb.timestep_embedder.linear_1", d, 256)
            lin(n + ".emb.timestep_embedder.linear_2", d, d)
            lin(n + ".linear", r * d, d)

        mods = [("", dv, self.in_channels, self.out_channels)]
        if self.is_av:
            mods.append(("audio_", da, self.AUDIO_IN_CHANNELS, self.AUDIO_OUT_CHANNELS))
        for pre, d, cin, cout in mods:
            lin(pre + "patchify_proj", d, cin)
            adaln(pre + "adaln_single", d, rows)
            if self.cross_attention_adaln:
                adaln(pre + "prompt_adaln_single", d, 2)
            if self.caption_channels:
                lin(pre + "caption_projection.linear_1", d, self.caption_channels)
                lin(pre + "caption_projection.linear_2", d, d)
            s[pre + "scale_shift_table"] = (2, d)
            lin(pre + "proj_out", cout, d)
        if self.is_av:
            adaln("av_ca_video_scale_shift_adaln_single", dv, 4)
            adaln("av_ca_a2v_gate_adaln_single", dv, 1)
            adaln("av_ca_audio_scale_shift_adaln_single", da, 4)
            adaln("av_ca_v2a_gate_adaln_single", da, 1)
        for i in range(self.num_layers):
            p = f"transformer_blocks.{i}"
            for name, dq, dc, di, heads, _ in self._attn_specs():
                lin(f"{p}.{name}.to_q", di, dq)
                lin(f"{p}.{name}.to_k", di, dc)
                lin(f"{p}.{name}.to_v", di, dc)
                lin(f"{p}.{name}.to_out.0", dq, di)
                s[f"{p}.{name}.q_norm.weight"] = (di,)
                s[f"{p}.{name}.k_norm.weight"] = (di,)
                if self.apply_gated_attention:
                    lin(f"{p}.{name}.to_gate_logits", heads, dq)
            for pre, d, _, _ in mods:
                lin(f"{p}.{pre}ff.net.0.proj", 4 * d, d)
                lin(f"{p}.{pre}ff.net.2", d, 4 * d)
                s[f"{p}.{pre}scale_shift_table"] = (rows, d)
                if self.cross_attention_adaln:
                    s[f"{p}.{pre}prompt_scale_shift_table"] = (2, d)
            if self.is_av:
                s[f"{p}.scale_shift_table_a2v_ca_audio"] = (5, da)
                s[f"{p}.scale_shift_table_a2v_ca_video"] = (5, dv)
        return s

    def _register(self, name: str, t: torch.Tensor) -> None:
        t = t.contiguous()
        self._w[name] = t
        # uint8 = float8_e4m3fn codes of an fp8-RESIDENT linear weight (its `<name>_scale` fp32 vector is registered with it)
        dt = nv.DTYPE_BF16 if t.dtype == self.compute_dtype else (nv.DTYPE_FP8_E4M3FN if t.dtype == torch.uint8 else nv.DTYPE_F32)
        if t.dtype in (BF16, torch.float16) and t.dtype != self.compute_dtype:
            raise ValueError(f"{name}: {t.dtype} weight registered with a {self.compute_dtype} model")
        nv.check(self._L.ltx2_dit_set_weight(self._h, name.encode(), nv.ptr(t), dt, t.numel()))

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True) -> None:
        """Consume checkpoint-keyed tensors (any float dtype, any device).  Linear weights stay
        [out, in] (no transposes, weight_converter.py:303-307) and become bf16; biases, norm
        weights and scale_shift_tables become fp32 (transformer.py:157-159).  q/k/v of the
        self-attentions and k/v of the cross-attentions are concatenated at load time for fused
        projection GEMMs."""
        exp = self.expected_weight_shapes()
        missing = [k for k in exp if k not in sd]
        if missing and strict:
            raise KeyError(f"missing {len(missing)} weights, e.g. {missing[:4]}")
        for k, shp in exp.items():
            if k in sd and tuple(sd[k].shape) != shp:
                raise ValueError(f"weight {k}: shape {tuple(sd[k].shape)} != expected {shp}")
        for k, v in sd.items():
            if isinstance(v, Fp8Weight) and not FP8_RESIDENT_KEYS.match(k):
                raise ValueError(f"{k}: only the video stream's attention / feed-forward projections can stay fp8-resident")
        ff_key = "transformer_blocks.0.ff.net.0.proj.weight"
        if ff_key in sd and sd[ff_key].shape[0] != 4 * self.inner_dim:
            raise ValueError("FFN must be the ungated Linear(D->4D) (reference feed_forward.py:29-54)")
        dev = self.device

        def W(name):
            return sd[name].to(dev, self.compute_dtype)

        def Fv(name):
            return sd[name].to(dev, torch.float32)

        def put_linear(dst, names):
            """Register the (possibly fused) linear weight `dst` from checkpoint tensors `names`.  Fp8Weight entries (codes +
            per-tensor scale, loader fp8_resident=True) stay fp8 in HBM: codes concatenated, one scale per output row."""
            vals = [sd[n] for n in names]
            if self.fp8_compute and all(FP8_RESIDENT_KEYS.match(n) for n in names) and not any(isinstance(v, Fp8Weight) for v in vals) \
                    and vals[0].shape[0] % 256 == 0 and vals[0].shape[1] % 256 == 0 and vals[0].shape[1] >= 512:
                # bf16 checkpoint + fp8 compute: one e4m3fn scale per OUTPUT CHANNEL (ltx2_quantize_rows_fp8, the activations' quantiser)
                q = [K.quantize_rows_fp8(v.to(dev, self.compute_dtype)) for v in vals]
                self._register(dst, torch.cat([c for c, _ in q], 0))
                self._register(dst + "_scale", torch.cat([s_ for _, s_ in q], 0))
                return
            if any(isinstance(v, Fp8Weight) for v in vals):
                if not all(isinstance(v, Fp8Weight) for v in vals):
                    raise ValueError(f"{dst}: fused projection mixes fp8-resident and dequantised parts")
                if vals[0].codes.shape[0] % 256 or vals[0].codes.shape[1] % 128 or vals[0].codes.shape[1] < 256:
                    raise ValueError(f"{dst}: fp8-resident weights need out % 256 == 0 and in % 128 == 0 (got {tuple(vals[0].codes.shape)})")
                self._register(dst, torch.cat([v.codes.to(dev).view(torch.uint8) for v in vals], 0))
                self._register(dst + "_scale", torch.cat([torch.full((v.codes.shape[0],), float(v.scale), dtype=torch.float32, device=dev) for v in vals]))
            else:
                self._register(dst, torch.cat([v.to(dev, self.compute_dtype) for v in vals], 0) if len(vals) > 1 else vals[0].to(dev, self.compute_dtype))

        fused = set()
        for i in range(self.num_layers):
            p = f"transformer_blocks.{i}"
            for name, _, _, _, _, is_self in self._attn_specs():
                parts = ("to_q", "to_k", "to_v") if is_self else ("to_k", "to_v")
                dst = "to_qkv" if is_self else "to_kv"
                if any(f"{p}.{name}.{n}.weight" not in sd for n in parts):
                    continue
                put_linear(f"{p}.{name}.{dst}.weight", [f"{p}.{name}.{n}.weight" for n in parts])
                self._register(f"{p}.{name}.{dst}.bias", torch.cat([Fv(f"{p}.{name}.{n}.bias") for n in parts], 0))
                fused.update(f"{p}.{name}.{n}" for n in parts)
        for k in exp:
            if k not in sd or k.rsplit(".", 1)[0] in fused:
                continue
            is_linear_w = k.endswith(".weight") and len(exp[k]) == 2
            if is_linear_w:
                put_linear(k, [k])
            else:
                self._register(k, Fv(k))
        self._prep_key = None
        self._twin = None           # contexts over the OLD tensors: rebuilt on demand over the new ones
        self._clone = None

    def init_random_weights(self, seed: int = 0, std: float = 0.02, fp8_resident: bool = False, fill: bool = True) -> None:
        """Synthetic N(0, std) weights generated directly in HBM in the engine's fused layout (bench /
        smoke; no checkpoints exist in this environment).  fp8_resident: the video stream's attention / feed-forward
        projections are quantised to float8_e4m3fn + per-tensor scale and stay fp8 in HBM (BASELINE config 3).
        fill=False: only ALLOCATE and register the tensors (same names, shapes, dtypes; contents undefined) -- a replica whose
        weights arrive by the RCCL broadcast from rank 0 (bench.py ranks > 0) does not draw 26 GB of random numbers first."""
        fp8_resident = fp8_resident or self.fp8_compute
        g = torch.Generator(device=self.device).manual_seed(seed)
        fused_fp8 = re.compile(r"^transformer_blocks\.\d+\.(attn1|attn2)\.(to_qkv|to_q|to_kv|to_out\.0)\.weight$|^transformer_blocks\.\d+\.ff\.net\.(0\.proj|2)\.weight$")

        def rw(*shape):
            if not fill:
                return torch.empty(*shape, device=self.device, dtype=self.compute_dtype)
            return (torch.randn(*shape, generator=g, device=self.device, dtype=torch.float32) * std).to(self.compute_dtype)

        def put_w(name, rows, cols):
            if fp8_resident and fused_fp8.match(name) and rows % 256 == 0 and cols % 128 == 0 and cols >= 256:
                if not fill:
                    self._register(name, torch.empty(rows, cols, device=self.device, dtype=torch.uint8))
                    self._register(name + "_scale", torch.empty(rows, dtype=torch.float32, device=self.device))
                    return
                w = torch.randn(rows, cols, generator=g, device=self.device, dtype=torch.float32) * std
                scale = float(w.abs().max() / 448.0)
                self._register(name, (w / scale).to(torch.float8_e4m3fn).view(torch.uint8))
                self._register(name + "_scale", torch.full((rows,), scale, dtype=torch.float32, device=self.device))
            else:
                self._register(name, rw(rows, cols))

        def rf(*shape, scale=std, base=0.0):
            if not fill:
                return torch.empty(*shape, device=self.device, dtype=torch.float32)
            return base + scale * torch.randn(*shape, generator=g, device=self.device, dtype=torch.float32)

        fuse = {}
        for name, _, _, _, _, is_self in self._attn_specs():
            fuse[name] = ("to_q", "to_k", "to_v") if is_self else ("to_k", "to_v")
        done = set()
        exp = self.expected_weight_shapes()
        for k, shp in exp.items():
            mod, leaf = k.rsplit(".", 1) if "." in k else ("", k)
            parent, last = mod.rsplit(".", 1) if "." in mod else ("", mod)
            attn = parent.rsplit(".", 1)[-1]
            if attn in fuse and last in fuse[attn]:
                dst = f"{parent}.{'to_qkv' if len(fuse[attn]) == 3 else 'to_kv'}.{leaf}"
                if dst in done:
                    continue
                done.add(dst)
                rows = sum(exp[f"{parent}.{n}.{leaf}"][0] for n in fuse[attn])
                if leaf == "weight":
                    put_w(dst, rows, shp[1])
                else:
                    self._register(dst, rf(rows))
            elif k.endswith("_norm.weight"):
                self._register(k, rf(*shp, scale=0.0, base=1.0))
            elif leaf == "weight" and len(shp) == 2:
                put_w(k, *shp)
            else:
                self._register(k, rf(*shp))
        self._prep_key = None
        self._twin = None
        self._clone = None

    def weight_tensors(self) -> Dict[str, torch.Tensor]:
        """Engine-layout device tensors (used by the RCCL weight broadcast)."""
        return self._w

    # ------------------------------------------------------------------ workspace / prepare
    def _bind(self, n: int, s: int, per_token: bool, na: int = 0, sa: int = 0) -> None:
        want = (n, s, na, sa, int(per_token))
        if self._bound[:4] == want[:4] and self._bound[4] >= want[4] and self._ws is not None:
            return
        L = self._L
        nbytes = (L.ltx2_dit_workspace_bytes_av(self._h, n, s, na, sa, int(per_token)) if self.is_av else
                  L.ltx2_dit_workspace_bytes(self._h, n, s, int(per_token)))
        if nbytes <= 0:
            raise ValueError(f"bad workspace request N={n} S={s} Na={na} Sa={sa}")
        self._ws = None
        self._ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        base = (self._ws.data_ptr() + 255) // 256 * 256
        if self.is_av:
            nv.check(L.ltx2_dit_bind_workspace_av(self._h, base, nbytes, n, s, na, sa, int(per_token)))
        else:
            nv.check(L.ltx2_dit_bind_workspace(self._h, base, nbytes, n, s, int(per_token)))
        self._bound = want
        self._prep_key = None
        self._mask_refs = {}            # binding clears the engine's context masks

    def prepare(self, context: torch.Tensor, positions: torch.Tensor, per_token: bool = False,
                audio_context: Optional[torch.Tensor] = None, audio_positions: Optional[torch.Tensor] = None) -> None:
        """Per-prompt setup: bind workspace, upload RoPE tables (self-attention and, for AudioVideo,
        the temporal cross-modal tables of model.py:320-344), run caption projection and the per-layer
        text cross-attention K/V projections (ltx2_dit_prepare / ltx2_dit_prepare_av)."""
        if context.shape[0] != 1 or positions.shape[0] != 1:
            raise ValueError("batch must be 1 (the reference hard-wires batch=1: pipelines/distilled.py:314)")
        n, s = positions.shape[2], context.shape[1]
        dev = self.device
        theta = self.positional_embedding_theta
        # the cache key names the CALLER's tensors (which _ensure_prepared sees again on the next step), not the device copies
        # made below; the originals are kept alive in _prep_refs so a data_ptr cannot be recycled under the key
        key = self._key(context, positions, audio_context, audio_positions)
        originals = (context, positions, audio_context, audio_positions)
        positions = positions.to(dev)
        cos, sin = K.rope_tables(positions, self.inner_dim, theta, self.positional_embedding_max_pos)
        ctx = context[0].to(dev, torch.float32).contiguous()
        if not self.is_av:
            self._bind(n, s, per_token)
            nv.check(self._L.ltx2_dit_prepare(self._h, nv.ptr(ctx), s, nv.ptr(cos), nv.ptr(sin), nv.stream()))
            self._prep_refs = (originals, positions, cos, sin, ctx)     # keep pointers alive / unaliased
        else:
            if audio_context is None or audio_positions is None:
                raise ValueError("AudioVideo model: audio context and positions are required")
            na, sa = audio_positions.shape[2], audio_context.shape[1]
            self._bind(n, s, per_token, na, sa)
            mp = [self.AUDIO_CROSS_PE_MAX_POS]
            da, ha = self.audio_inner_dim, self.audio_heads
            audio_positions = audio_positions.to(dev)
            acos, asin = K.rope_tables(audio_positions, da, theta, mp)
            vcc, vcs = K.rope_tables(positions[:, 0:1], da, theta, mp)
            acc, acs = K.rope_tables(audio_positions[:, 0:1], da, theta, mp)
            actx = audio_context[0].to(dev, torch.float32).contiguous()
            nv.check(self._L.ltx2_dit_prepare_av(self._h, nv.ptr(ctx), s, nv.ptr(cos), nv.ptr(sin), nv.ptr(vcc), nv.ptr(vcs),
                                                  nv.ptr(actx), sa, nv.ptr(acos), nv.ptr(asin), nv.ptr(acc), nv.ptr(acs),
                                                  nv.stream()))
            self._prep_refs = (originals, positions, audio_positions, cos, sin, ctx, acos, asin, vcc, vcs, acc, acs, actx)
        self._prep_key = key

    @staticmethod
    def _key(context, positions, audio_context=None, audio_positions=None):
        def one(t):
            return None if t is None else (t.data_ptr(), t._version, tuple(t.shape), t.dtype)
        return (one(context), one(positions), one(audio_context), one(audio_positions))

    def _ensure_prepared(self, video: Modality, per_token: bool, audio: Optional[Modality] = None) -> None:
        key = self._key(video.context, video.positions, audio.context if audio else None, audio.positions if audio else None)
        if self._prep_key != key or (per_token and not self._bound[4]):
            self.prepare(video.context, video.positions, per_token=per_token,
                         audio_context=audio.context if audio else None, audio_positions=audio.positions if audio else None)

    # ------------------------------------------------------------------ forward
    def _timesteps(self, m: Modality) -> Tuple[torch.Tensor, int]:
        """-> (fp32 device vector, n_timesteps in {1, N}).  A 1-element tensor (shape (B,), what every pipeline here passes when no
        token carries a conditioning mask -- `modality_from_state(..., uniform=True)`) takes the broadcast AdaLN path; N timesteps
        (shape (B, N) / (B, N, 1), the reference's `denoise_mask * sigma`) ALWAYS take the per-token path, equal or not: identical
        arithmetic, N x more AdaLN MLP rows -- asking the device whether they happen to be equal would be a host sync per step.  A
        caller that knows its mask is all ones should pass the scalar form."""
        ts = m.timesteps.to(self.device, torch.float32).reshape(-1).contiguous()
        n = m.latent.shape[1]
        if ts.numel() == 1:
            return ts, 1
        if ts.numel() != n:
            raise ValueError(f"timesteps has {ts.numel()} elements; expected 1 or N={n}")
        # per-token timesteps stay per-token: asking the device whether they happen to be equal would be a host sync on
        # every step (uniform sigma arrives as a 1-element tensor from every pipeline that has no conditioning mask)
        return ts, n

    def _sigma(self, m: Modality) -> torch.Tensor:
        """Modality.sigma, or the first timestep when absent (model.py:154-156,393-395)."""
        s = m.sigma if m.sigma is not None else m.timesteps
        return s.to(self.device, torch.float32).reshape(-1)[:1].contiguous()

    def _check_inputs(self, video, audio, perturbations):
        if video is None:
            raise ValueError("Video modality required for video-enabled model")     # model.py:823-824
        for m in (video, audio):
            if m is not None and m.context_mask is not None:
                cm = m.context_mask
                if cm.dtype.is_floating_point:
                    # model.py:186-187 hands a float mask to the attention as an ADDITIVE bias of any shape; no reference path builds one
                    raise NotImplementedError("float (additive) context_mask: pass the boolean (B, S) key mask instead")
                if cm.dim() != 2 or cm.shape[0] != 1 or cm.shape[1] != m.context.shape[1]:
                    raise ValueError(f"context_mask must be (1, S={m.context.shape[1]}); got {tuple(cm.shape)}")
            if m is not None and m.latent.shape[0] != 1:
                raise ValueError("batch must be 1")
        if not self.is_av and audio is not None:
            raise ValueError("audio modality passed to a VideoOnly model")

    def __call__(self, video: Optional[Modality] = None, audio: Optional[Modality] = None, perturbations=None):
        """perturbations: a BatchedPerturbationConfig of batch 1 -- the forward then skips the self-attentions it names (the engine's perturbed
        entries; the config holds for this call alone, the sets of set_stg_blocks are back when it returns).  None or an empty config: the plain
        forward."""
        self._check_inputs(video, audio, perturbations)
        flags = self._perturbation_flags(perturbations)
        if self.is_av and (audio is None or not audio.enabled or audio.latent.shape[1] == 0):     # transformer.py:480: run_ax needs audio.enabled and tokens
            # video-only inference on an AudioVideo model (model.py:829-840, 866-874): (video velocity, empty audio output)
            v = self._video_twin()(video, None, perturbations=perturbations)
            return v, torch.zeros(1, 0, self.AUDIO_OUT_CHANNELS, device=self.device)
        ts, n_ts = self._timesteps(video)
        lat = video.latent[0].to(self.device, torch.float32).contiguous()
        out = torch.empty(lat.shape[0], self.out_channels, device=self.device, dtype=torch.float32)
        if not self.is_av:
            self._ensure_prepared(video, per_token=(n_ts != 1))
            self._apply_context_masks(video)
            # prompt AdaLN (V2.3) takes Modality.sigma, not timesteps[0]: with image conditioning timesteps = mask * sigma
            sg = self._sigma(video) if self.cross_attention_adaln else None
            if flags is None:
                nv.check(self._L.ltx2_dit_forward(self._h, nv.ptr(lat), nv.ptr(ts), n_ts, nv.ptr(sg), nv.ptr(out), nv.stream()))
            else:
                with self._stg_override(flags):
                    nv.check(self._L.ltx2_dit_forward_perturbed(self._h, nv.ptr(lat), nv.ptr(ts), n_ts, nv.ptr(sg), nv.ptr(out), nv.stream()))
            return out[None]
        ats, n_ats = self._timesteps(audio)
        self._ensure_prepared(video, per_token=(n_ts != 1 or n_ats != 1), audio=audio)
        self._apply_context_masks(video, audio)
        alat = audio.latent[0].to(self.device, torch.float32).contiguous()
        aout = torch.empty(alat.shape[0], self.AUDIO_OUT_CHANNELS, device=self.device, dtype=torch.float32)
        vs, as_ = self._sigma(video), self._sigma(audio)
        args = (self._h, nv.ptr(lat), nv.ptr(ts), n_ts, nv.ptr(vs), nv.ptr(alat), nv.ptr(ats), n_ats, nv.ptr(as_), nv.ptr(out), nv.ptr(aout), nv.stream())
        if flags is None:
            nv.check(self._L.ltx2_dit_forward_av(*args))
        else:
            with self._stg_override(flags):
                nv.check(self._L.ltx2_dit_forward_perturbed_av(*args))
        return out[None], aout[None]

    def _apply_context_masks(self, video: Modality, audio: Optional[Modality] = None) -> None:
        """Modality.context_mask -> the engine's text cross-attention key mask (ltx2_dit_set_context_mask; model.py:163-201 +
        attention.py:38-70).  After _ensure_prepared: binding a workspace clears the engine's masks."""
        for k, m in enumerate((video, audio)):
            if m is None:
                continue
            if m.context_mask is None:
                if self._mask_refs.get(k) is not None:
                    nv.check(self._L.ltx2_dit_set_context_mask(self._h, k, None, 0, nv.stream()))
                    self._mask_refs[k] = None
                continue
            f = (m.context_mask[0].to(self.device) != 0).to(torch.float32).contiguous()
            nv.check(self._L.ltx2_dit_set_context_mask(self._h, k, nv.ptr(f), f.numel(), nv.stream()))
            self._mask_refs[k] = f

    def _sigma_scalar(self, sigma: float) -> torch.Tensor:
        t = self._sigma_dev.get(float(sigma))
        if t is None:
            if len(self._sigma_dev) > 256:
                self._sigma_dev.clear()
            t = self._sigma_dev[float(sigma)] = torch.tensor([float(sigma)], device=self.device, dtype=torch.float32)
        return t

    # ------------------------------------------------------------------ fused sampling step / graph
    def _step_inputs(self, latent: torch.Tensor, video: Modality, sigma: float, audio_latent: Optional[torch.Tensor] = None,
                     audio: Optional[Modality] = None):
        """What every fused step does first: -> (timesteps, n_timesteps, the prompt AdaLN's sigma scalar or None), with this context prepared
        for `video` and its context mask applied.  On an AudioVideo context, with `audio`: -> (timesteps, n_timesteps, the sigma scalar both
        modalities share, audio timesteps, n_audio_timesteps), prepared for both modalities."""
        ts, n_ts = self._timesteps(video)
        assert latent.dtype == torch.float32 and latent.is_contiguous() and latent.dim() == 2
        if not self.is_av:
            self._ensure_prepared(video, per_token=(n_ts != 1))
            self._apply_context_masks(video)
            return ts, n_ts, (self._sigma_scalar(sigma) if self.cross_attention_adaln else None)
        assert audio is not None and audio_latent is not None and audio_latent.dtype == torch.float32 and audio_latent.is_contiguous()
        ats, n_ats = self._timesteps(audio)
        self._ensure_prepared(video, per_token=(n_ts != 1 or n_ats != 1), audio=audio)
        self._apply_context_masks(video, audio)
        return ts, n_ts, self._sigma_scalar(sigma), ats, n_ats

    def _capture_inputs(self, sigmas: Sequence[float], *mask_clean_pairs):
        """What every capture_*_graph does first: -> (the sigmas as a c_float array, the step count, the current stream, n_el).  Capture
        needs a non-default stream; every (denoise_mask, clean_latent) pair must be fp32 and contiguous, the mask one-dimensional.  n_el(t)
        is a buffer's element count (0 for None): the engine checks it against the bound token count, as a wrong-length buffer would be an
        out-of-bounds read on replay."""
        arr = (C.c_float * len(sigmas))(*[float(s) for s in sigmas])
        st = torch.cuda.current_stream()
        if st.cuda_stream == 0:
            raise RuntimeError("graph capture needs a non-default stream: use `with torch.cuda.stream(torch.cuda.Stream()):`")
        for mk, cl in mask_clean_pairs:
            if mk is not None:
                assert cl is not None and mk.dtype == torch.float32 and cl.dtype == torch.float32 and mk.is_contiguous() and cl.is_contiguous() and mk.dim() == 1
        return arr, len(sigmas) - 1, st, (lambda t: 0 if t is None else t.numel())

    def _replay(self, kind: str, missing: str) -> None:
        """Launch the graph of the last capture of `kind` made through this object, on the context that holds it."""
        if self._graph_owner is None or self._graph_owner[0] != kind:
            raise RuntimeError(missing)
        owner = self._graph_owner[1]
        nv.check(owner._L.ltx2_dit_graph_launch(owner._h, nv.stream()))

    def denoise_step_(self, latent: torch.Tensor, video: Modality, sigma: float, sigma_next: float,
                      denoise_mask: Optional[torch.Tensor] = None, clean_latent: Optional[torch.Tensor] = None,
                      audio_latent: Optional[torch.Tensor] = None, audio: Optional[Modality] = None,
                      audio_denoise_mask: Optional[torch.Tensor] = None, audio_clean_latent: Optional[torch.Tensor] = None) -> None:
        """In-place: latent (N, C) fp32 <- Euler(latent, post_process(x0)) -- forward + x0 + blend + step
        enqueued by ONE C call (ltx2_dit_denoise_step / _av; the AudioVideo form updates both latents)."""
        if not self.is_av:
            ts, n_ts, sg = self._step_inputs(latent, video, sigma)
            nv.check(self._L.ltx2_dit_denoise_step(self._h, nv.ptr(latent), nv.ptr(ts), n_ts, nv.ptr(sg), nv.ptr(denoise_mask),
                                                    nv.ptr(clean_latent), float(sigma), float(sigma_next), None, nv.stream()))
            return
        ts, n_ts, sg, ats, n_ats = self._step_inputs(latent, video, sigma, audio_latent, audio)
        nv.check(self._L.ltx2_dit_denoise_step_av(self._h, nv.ptr(latent), nv.ptr(audio_latent), nv.ptr(ts), n_ts, nv.ptr(ats), n_ats,
                                                   nv.ptr(sg), nv.ptr(denoise_mask), nv.ptr(clean_latent), nv.ptr(audio_denoise_mask),
                                                   nv.ptr(audio_clean_latent), float(sigma), float(sigma_next), None, None, nv.stream()))

    def capture_denoise_graph(self, latent: torch.Tensor, sigmas: Sequence[float], audio_latent: Optional[torch.Tensor] = None,
                              denoise_mask: Optional[torch.Tensor] = None, clean_latent: Optional[torch.Tensor] = None,
                              audio_denoise_mask: Optional[torch.Tensor] = None, audio_clean_latent: Optional[torch.Tensor] = None) -> None:
        """hipGraph-capture len(sigmas)-1 steps over `latent` (N, C fp32; plus the audio latent for
        AudioVideo models), updated in place on replay.  denoise_mask (N,) fp32 + clean_latent (N, C) fp32 (per modality): the CONDITIONED
        loop of image-to-video runs -- per-token timesteps mask * sigma_i and the x0 / clean blend inside every captured step
        (ltx2_dit_graph_capture_cond; prepare(..., per_token=True) first).  The tensors must stay alive while the graph is replayed."""
        assert self._prep_key is not None, "call prepare() first"
        arr, n, st, n_el = self._capture_inputs(sigmas, (denoise_mask, clean_latent), (audio_denoise_mask, audio_clean_latent))
        cond = denoise_mask is not None or audio_denoise_mask is not None
        self._graph_refs = (latent, audio_latent, denoise_mask, clean_latent, audio_denoise_mask, audio_clean_latent)
        self._graph_owner = ("denoise", self)
        if self.is_av:
            assert audio_latent is not None
            if cond:
                nv.check(self._L.ltx2_dit_graph_capture_cond_av(self._h, nv.ptr(latent), nv.ptr(audio_latent), arr, n, nv.ptr(denoise_mask), n_el(denoise_mask),
                                                                nv.ptr(clean_latent), n_el(clean_latent), nv.ptr(audio_denoise_mask), n_el(audio_denoise_mask),
                                                                nv.ptr(audio_clean_latent), n_el(audio_clean_latent), st.cuda_stream))
            else:
                nv.check(self._L.ltx2_dit_graph_capture_av(self._h, nv.ptr(latent), nv.ptr(audio_latent), arr, n, st.cuda_stream))
        elif cond:
            nv.check(self._L.ltx2_dit_graph_capture_cond(self._h, nv.ptr(latent), arr, n, nv.ptr(denoise_mask), n_el(denoise_mask), nv.ptr(clean_latent), n_el(clean_latent), st.cuda_stream))
        else:
            nv.check(self._L.ltx2_dit_graph_capture(self._h, nv.ptr(latent), arr, n, st.cuda_stream))

    # ------------------------------------------------------------------ guided and second-order steps: what they share
    def _contexts(self, neg: Optional["LTXModel"], av: bool = False, optional: bool = False) -> Tuple["LTXModel", Optional["LTXModel"]]:
        """(positive, negative) contexts of a guided step.  av=False: VideoOnly contexts, an AudioVideo model used through its video twin;
        av=True: AudioVideo contexts, as they are.  optional: neg may be None (a step that also runs without guidance) and is returned so."""
        if not (isinstance(neg, LTXModel) or (optional and neg is None)):
            raise ValueError("guidance needs a second LTXModel context (clone_sharing_weights()) for the negative prompt")
        if av:
            if not (self.is_av and (neg is None or neg.is_av)):
                raise ValueError("the *_av_ steps run on AudioVideo contexts (a VideoOnly model has the step without _av)")
            return self, neg
        return (self._video_twin() if self.is_av else self), (neg._video_twin() if neg is not None and neg.is_av else neg)

    def _capture(self, kind: str, pos: "LTXModel", ng: Optional["LTXModel"], symbol: str, refs: tuple, sigmas: Sequence[float], mask_clean_pairs, *tail) -> None:
        """What every guided capture_*_graph does: the C call `symbol`(pos, ng, the latents `refs`, sigmas, n, the video conditioning
        mask_clean_pairs[0], *tail, stream) -- a tensor or None goes as (pointer, element count), further pairs are only checked (the frozen
        audio's mask travels in tail) -- with the graph, and every tensor it reads, kept by `pos` and replayed as `kind`."""
        assert pos._prep_key is not None and (ng is None or ng._prep_key is not None), "call prepare() on both contexts first"
        arr, n, st, n_el = self._capture_inputs(sigmas, *mask_clean_pairs)
        is_buf = lambda a: a is None or isinstance(a, torch.Tensor)      # noqa: E731
        args = [x for a in (*mask_clean_pairs[0], *tail) for x in ((nv.ptr(a), n_el(a)) if is_buf(a) else (a,))]
        pos._graph_refs = (*refs, *(t for pair in mask_clean_pairs for t in pair), *(a for a in tail if is_buf(a)), ng)
        nv.check(getattr(pos._L, symbol)(pos._h, None if ng is None else ng._h, *(nv.ptr(t) for t in refs), arr, n, *args, st.cuda_stream))
        self._graph_owner = (kind, pos)

    # ------------------------------------------------------------------ classifier-free guidance (video-only engine)
    def guided_step_(self, neg: "LTXModel", latent: torch.Tensor, video: Modality, sigma: float, sigma_next: float, cfg_scale: float,
                     denoise_mask: Optional[torch.Tensor] = None, clean_latent: Optional[torch.Tensor] = None) -> None:
        """In-place: latent (N, C) fp32 <- one classifier-free-guided Euler step -- the positive prompt through this context, the negative one
        through `neg` (clone_sharing_weights(), prepared by the caller with the negative context), then x0 x 2 + CFGGuider.guide +
        post_process_latent + Euler in one kernel, all enqueued by ONE C call (ltx2_dit_guided_step)."""
        pos, ng = self._contexts(neg)
        ts, n_ts, sg = pos._step_inputs(latent, video, sigma)
        nv.check(pos._L.ltx2_dit_guided_step(pos._h, ng._h, nv.ptr(latent), nv.ptr(ts), n_ts, nv.ptr(sg), nv.ptr(denoise_mask), nv.ptr(clean_latent),
                                             float(cfg_scale), float(sigma), float(sigma_next), nv.stream()))

    def capture_guided_graph(self, neg: "LTXModel", latent: torch.Tensor, sigmas: Sequence[float], cfg_scale: float,
                             denoise_mask: Optional[torch.Tensor] = None, clean_latent: Optional[torch.Tensor] = None) -> None:
        """hipGraph-capture len(sigmas)-1 guided steps over `latent` (N, C fp32), a linear chain of forward(self), forward(neg) and the guided
        Euler kernel per step (ltx2_dit_graph_capture_guided).  Both contexts are prepared first (per_token=True when a mask is given); the
        graph belongs to the positive VideoOnly context (this one, or an AudioVideo model's video twin) and replay_guided_graph() replays
        it.  The tensors must stay alive while it is replayed."""
        pos, ng = self._contexts(neg)
        self._capture("guided", pos, ng, "ltx2_dit_graph_capture_guided", (latent,), sigmas, [(denoise_mask, clean_latent)], float(cfg_scale))

    def replay_guided_graph(self) -> None:
        """Replay the graph captured by capture_guided_graph (it belongs to the VideoOnly context that ran the capture)."""
        self._replay("guided", "no guided graph captured")

    # ------------------------------------------------------------------ CFG with the per-channel rescale: the standard one-stage loop (video-only engine)
    def rescaled_guided_step_(self, neg: "LTXModel", latent: torch.Tensor, video: Modality, sigma: float, sigma_next: float, cfg_scale: float,
                              guidance_rescale: float) -> None:
        """In-place: latent (N, C) fp32 <- one guided step of the reference's standard one-stage loop by ONE C call
        (ltx2_dit_rescaled_guided_step): forward(self), forward(neg), g = uncond + cfg_scale*(cond - uncond) on the x0 predictions, with
        guidance_rescale > 0 the per-channel statistics and rescale_noise_cfg, then the Euler update.  No conditioning on this route."""
        pos, ng = self._contexts(neg)
        ts, n_ts, sg = pos._step_inputs(latent, video, sigma)
        nv.check(pos._L.ltx2_dit_rescaled_guided_step(pos._h, ng._h, nv.ptr(latent), nv.ptr(ts), n_ts, nv.ptr(sg), float(cfg_scale), float(guidance_rescale),
                                                      float(sigma), float(sigma_next), nv.stream()))

    def capture_rescaled_guided_graph(self, neg: "LTXModel", latent: torch.Tensor, sigmas: Sequence[float], cfg_scale: float,
                                      guidance_rescale: float) -> None:
        """hipGraph-capture len(sigmas)-1 of those steps over `latent` (N, C fp32) with uniform timesteps, one linear chain
        (ltx2_dit_graph_capture_rescaled_guided).  Both contexts are prepared first; the graph belongs to the positive VideoOnly context and
        replay_rescaled_guided_graph() replays it.  The latent must stay alive while it is replayed."""
        pos, ng = self._contexts(neg)
        assert pos._prep_key is not None and ng._prep_key is not None, "call prepare() on both contexts first"
        arr, n, st, _ = self._capture_inputs(sigmas)
        pos._graph_refs = (latent, ng)
        nv.check(pos._L.ltx2_dit_graph_capture_rescaled_guided(pos._h, ng._h, nv.ptr(latent), arr, n, float(cfg_scale), float(guidance_rescale),
                                                               st.cuda_stream))
        self._graph_owner = ("rescaled_guided", pos)

    def replay_rescaled_guided_graph(self) -> None:
        """Replay the graph captured by capture_rescaled_guided_graph (it belongs to the VideoOnly context that ran the capture)."""
        self._replay("rescaled_guided", "no rescaled guided graph captured")

    # ------------------------------------------------------------------ first-block cache (video-only engine, opt-in)
    def enable_first_block_cache(self, threshold: float, slots: int = 2) -> None:
        """Turn the first-block cache on for this context (ltx2_dit_fbc_configure): `slots` cache slots, one per kind of evaluation within a
        step, and the threshold t of the skip test sum|r - head_prev| < t * sum|head_prev| on block 0's residual r.  The cached entries
        (forward_cached, denoise_step_cached_, rescaled_guided_step_cached_) then reuse the stored residual of blocks 1..L-1 where the test
        holds; every other entry is untouched.  slots=0 turns it off and frees the buffers ((2*slots + 2) fp32 [N, D] buffers).  A negative
        threshold is a ValueError; an AudioVideo model is refused."""
        if not float(threshold) >= 0.0:
            raise ValueError(f"first_block_cache threshold={threshold!r} must be >= 0")
        if self.is_av:
            raise NotImplementedError("the first-block cache is built for the video-only model alone (AudioVideo / LTX-2.3 joint models are outside it)")
        nv.check(self._L.ltx2_dit_fbc_configure(self._h, int(slots), float(threshold)))
        self._fbc = (float(threshold), int(slots))

    def reset_first_block_cache(self) -> None:
        """Every slot invalid, its counts zero (ltx2_dit_fbc_reset): what a loop does at its start."""
        nv.check(self._L.ltx2_dit_fbc_reset(self._h))

    def force_first_block_cache(self, slot: int = -1) -> None:
        """The next cached evaluation in `slot` (-1: in every slot) computes in full (ltx2_dit_fbc_force_next): a loop's last step."""
        nv.check(self._L.ltx2_dit_fbc_force_next(self._h, int(slot)))

    def first_block_cache_stats(self) -> List[Dict[str, float]]:
        """Per slot: evaluations and skips since the last reset, and num / den of the last evaluation that read its metric back."""
        out = []
        for k in range(getattr(self, "_fbc", (0.0, 0))[1]):
            ev, sk, num, den = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
            nv.check(self._L.ltx2_dit_fbc_stats(self._h, k, C.byref(ev), C.byref(sk), C.byref(num), C.byref(den)))
            out.append(dict(evaluations=ev.value, skips=sk.value, last_num=num.value, last_den=den.value))
        return out

    def forward_cached(self, video: Modality, slot: int = 0, perturbations=None) -> torch.Tensor:
        """__call__(video) of the video-only model through cache slot `slot` (ltx2_dit_forward_fbc).  A perturbed (STG) pass has no cached form."""
        self._check_inputs(video, None, perturbations)
        if self.is_av:
            raise NotImplementedError("the first-block cache is built for the video-only model alone (AudioVideo / LTX-2.3 joint models are outside it)")
        kind = 0 if self._perturbation_flags(perturbations) is None else 1
        ts, n_ts = self._timesteps(video)
        lat = video.latent[0].to(self.device, torch.float32).contiguous()
        out = torch.empty(lat.shape[0], self.out_channels, device=self.device, dtype=torch.float32)
        self._ensure_prepared(video, per_token=(n_ts != 1))
        self._apply_context_masks(video)
        sg = self._sigma(video) if self.cross_attention_adaln else None
        nv.check(self._L.ltx2_dit_forward_fbc(self._h, int(slot), kind, nv.ptr(lat), nv.ptr(ts), n_ts, nv.ptr(sg), nv.ptr(out), nv.stream()))
        return out[None]

    def denoise_step_cached_(self, latent: torch.Tensor, video: Modality, sigma: float, sigma_next: float, slot: int = 0) -> None:
        """denoise_step_ of the video-only model without conditioning, its forward through cache slot `slot` (ltx2_dit_denoise_step_fbc)."""
        if self.is_av:
            raise NotImplementedError("the first-block cache is built for the video-only model alone (AudioVideo / LTX-2.3 joint models are outside it)")
        ts, n_ts, sg = self._step_inputs(latent, video, sigma)
        nv.check(self._L.ltx2_dit_denoise_step_fbc(self._h, int(slot), nv.ptr(latent), nv.ptr(ts), n_ts, nv.ptr(sg), float(sigma), float(sigma_next),
                                                    nv.stream()))

    def rescaled_guided_step_cached_(self, neg: "LTXModel", latent: torch.Tensor, video: Modality, sigma: float, sigma_next: float, cfg_scale: float,
                                     guidance_rescale: float, slots: Tuple[int, int] = (0, 1)) -> None:
        """rescaled_guided_step_ with the positive pass through this context's cache slot slots[0] and the negative pass, on `neg`, through this
        context's slot slots[1] (ltx2_dit_rescaled_guided_step_fbc).  Eager only: each pass reads its decision back."""
        if self.is_av or neg.is_av:
            raise NotImplementedError("the first-block cache is built for the video-only model alone (AudioVideo / LTX-2.3 joint models are outside it)")
        pos, ng = self._contexts(neg)
        ts, n_ts, sg = pos._step_inputs(latent, video, sigma)
        nv.check(pos._L.ltx2_dit_rescaled_guided_step_fbc(pos._h, ng._h, int(slots[0]), int(slots[1]), nv.ptr(latent), nv.ptr(ts), n_ts, nv.ptr(sg),
                                                          float(cfg_scale), float(guidance_rescale), float(sigma), float(sigma_next), nv.stream()))

    # ------------------------------------------------------------------ spatio-temporal guidance on top of CFG (video-only engine)
    def stg_step_(self, neg: Optional["LTXModel"], latent: torch.Tensor, video: Modality, sigma: float, sigma_next: float, cfg_scale: float,
                  stg_scale: float, vel_perturbed: torch.Tensor, denoise_mask: Optional[torch.Tensor] = None,
                  clean_latent: Optional[torch.Tensor] = None) -> None:
        """In-place: latent (N, C) fp32 <- one Euler step under CFGGuider and STGGuider by ONE C call (ltx2_dit_stg_step): forward(self),
        forward(neg) (neg None: no CFG), a perturbed forward on this context itself -- the self-attentions of set_stg_blocks skipped -- into
        vel_perturbed (N, C fp32, the caller's scratch), then x0 x 3 + both guiders + post_process_latent + Euler in one kernel."""
        pos, ng = self._contexts(neg, optional=True)
        ts, n_ts, sg = pos._step_inputs(latent, video, sigma)
        assert vel_perturbed.dtype == torch.float32 and vel_perturbed.is_contiguous() and vel_perturbed.shape == latent.shape
        nv.check(pos._L.ltx2_dit_stg_step(pos._h, None if ng is None else ng._h, nv.ptr(latent), nv.ptr(ts), n_ts, nv.ptr(sg), nv.ptr(denoise_mask),
                                          nv.ptr(clean_latent), nv.ptr(vel_perturbed), float(cfg_scale), float(stg_scale), float(sigma),
                                          float(sigma_next), nv.stream()))

    def capture_stg_graph(self, neg: Optional["LTXModel"], latent: torch.Tensor, sigmas: Sequence[float], cfg_scale: float, stg_scale: float,
                          vel_perturbed: torch.Tensor, stg_cutoff: float = 1.0, denoise_mask: Optional[torch.Tensor] = None,
                          clean_latent: Optional[torch.Tensor] = None) -> None:
        """hipGraph-capture len(sigmas)-1 steps over `latent` (N, C fp32) as one linear chain (ltx2_dit_graph_capture_stg): step i is an STG
        step while (i + 1) / n <= stg_cutoff, then the guided step (the plain one when neg is None).  Both contexts are prepared first
        (per_token=True when a mask is given); the graph belongs to the positive VideoOnly context and replay_stg_graph() replays it.  The
        tensors must stay alive while it is replayed."""
        pos, ng = self._contexts(neg, optional=True)
        assert vel_perturbed.dtype == torch.float32 and vel_perturbed.is_contiguous()
        self._capture("stg", pos, ng, "ltx2_dit_graph_capture_stg", (latent,), sigmas, [(denoise_mask, clean_latent)], vel_perturbed,
                      float(cfg_scale), float(stg_scale), float(stg_cutoff))

    def replay_stg_graph(self) -> None:
        """Replay the graph captured by capture_stg_graph (it belongs to the VideoOnly context that ran the capture)."""
        self._replay("stg", "no STG graph captured")

    # ------------------------------------------------------------------ classifier-free guidance with a frozen audio latent (AudioVideo engine)
    def guided_step_av_(self, neg: "LTXModel", latent: torch.Tensor, audio_latent: torch.Tensor, video: Modality, audio: Modality, sigma: float,
                        sigma_next: float, cfg_scale: float, denoise_mask: Optional[torch.Tensor] = None,
                        clean_latent: Optional[torch.Tensor] = None) -> None:
        """In-place on the VIDEO latent (N, C) fp32: one classifier-free-guided Euler step of the AudioVideo model with the audio latent
        (Na, C) fp32 frozen -- both modalities through this context and through `neg` (clone_sharing_weights(), prepared by the caller with the
        negative contexts), then x0 x 2 + CFGGuider.guide + post_process_latent + Euler on the video alone, all enqueued by ONE C call
        (ltx2_dit_guided_step_av).  audio_latent is only read."""
        pos, ng = self._contexts(neg, av=True)
        ts, n_ts, sg, ats, n_ats = pos._step_inputs(latent, video, sigma, audio_latent, audio)
        nv.check(pos._L.ltx2_dit_guided_step_av(pos._h, ng._h, nv.ptr(latent), nv.ptr(audio_latent), nv.ptr(ts), n_ts, nv.ptr(ats), n_ats, nv.ptr(sg),
                                                nv.ptr(denoise_mask), nv.ptr(clean_latent), float(cfg_scale), float(sigma), float(sigma_next),
                                                nv.stream()))

    def capture_guided_av_graph(self, neg: "LTXModel", latent: torch.Tensor, audio_latent: torch.Tensor, sigmas: Sequence[float], cfg_scale: float,
                                denoise_mask: Optional[torch.Tensor] = None, clean_latent: Optional[torch.Tensor] = None,
                                audio_denoise_mask: Optional[torch.Tensor] = None) -> None:
        """hipGraph-capture len(sigmas)-1 of those steps over `latent` (N, C fp32), reading `audio_latent` (Na, C fp32) on every replay
        (ltx2_dit_graph_capture_guided_av).  audio_denoise_mask (Na,) fp32: the frozen audio's all-zero mask, its per-token timesteps.  Both
        contexts are prepared first (per_token=True when a mask is given); the graph belongs to this context and replay_guided_av_graph()
        replays it.  The tensors must stay alive while it is replayed."""
        pos, ng = self._contexts(neg, av=True)
        assert audio_latent.dtype == torch.float32 and audio_latent.is_contiguous()
        self._capture("guided_av", pos, ng, "ltx2_dit_graph_capture_guided_av", (latent, audio_latent), sigmas,
                      [(denoise_mask, clean_latent), (audio_denoise_mask, audio_latent)], audio_denoise_mask, float(cfg_scale))

    def replay_guided_av_graph(self) -> None:
        """Replay the graph captured by capture_guided_av_graph."""
        self._replay("guided_av", "no guided AudioVideo graph captured")

    # ------------------------------------------------------------------ classifier-free guidance on both latents (AudioVideo engine)
    def guided_step_joint_av_(self, neg: "LTXModel", latent: torch.Tensor, audio_latent: torch.Tensor, video: Modality, audio: Modality, sigma: float,
                              sigma_next: float, cfg_scale: float, audio_cfg_scale: float, denoise_mask: Optional[torch.Tensor] = None,
                              clean_latent: Optional[torch.Tensor] = None, audio_denoise_mask: Optional[torch.Tensor] = None,
                              audio_clean_latent: Optional[torch.Tensor] = None) -> None:
        """In-place on BOTH latents, (N, C) and (Na, Ca) fp32: one classifier-free-guided Euler step of the AudioVideo model (a retake with
        sound) by ONE C call (ltx2_dit_guided_step_joint_av): both modalities through this context and through `neg`, then x0 x 2 +
        CFGGuider.guide + post_process_latent + Euler over both latents in one launch, the video under cfg_scale and the audio under
        audio_cfg_scale.  Both contexts are prepared by the caller (neg with the negative contexts)."""
        pos, ng = self._contexts(neg, av=True)
        ts, n_ts, sg, ats, n_ats = pos._step_inputs(latent, video, sigma, audio_latent, audio)
        nv.check(pos._L.ltx2_dit_guided_step_joint_av(pos._h, ng._h, nv.ptr(latent), nv.ptr(audio_latent), nv.ptr(ts), n_ts, nv.ptr(ats), n_ats,
                                                      nv.ptr(sg), nv.ptr(denoise_mask), nv.ptr(clean_latent), nv.ptr(audio_denoise_mask),
                                                      nv.ptr(audio_clean_latent), float(cfg_scale), float(audio_cfg_scale), float(sigma),
                                                      float(sigma_next), nv.stream()))

    def capture_guided_joint_graph(self, neg: "LTXModel", latent: torch.Tensor, audio_latent: torch.Tensor, sigmas: Sequence[float], cfg_scale: float,
                                   audio_cfg_scale: float, denoise_mask: Optional[torch.Tensor] = None, clean_latent: Optional[torch.Tensor] = None,
                                   audio_denoise_mask: Optional[torch.Tensor] = None, audio_clean_latent: Optional[torch.Tensor] = None) -> None:
        """hipGraph-capture len(sigmas)-1 of those steps over both latents, updated in place on replay
        (ltx2_dit_graph_capture_guided_joint_av).  A modality with a denoise mask (and its clean latent) gets its per-token timesteps
        mask * sigma_i formed on the device.  Both contexts are prepared first (per_token=True when a mask is given); the graph belongs to
        this context and replay_guided_joint_graph() replays it.  The tensors must stay alive while it is replayed."""
        pos, ng = self._contexts(neg, av=True)
        assert audio_latent.dtype == torch.float32 and audio_latent.is_contiguous()
        self._capture("guided_joint", pos, ng, "ltx2_dit_graph_capture_guided_joint_av", (latent, audio_latent), sigmas,
                      [(denoise_mask, clean_latent), (audio_denoise_mask, audio_clean_latent)], audio_denoise_mask, audio_clean_latent,
                      float(cfg_scale), float(audio_cfg_scale))

    def replay_guided_joint_graph(self) -> None:
        """Replay the graph captured by capture_guided_joint_graph."""
        self._replay("guided_joint", "no joint guided graph captured")

    # ------------------------------------------------------------------ the Euler-ancestral step: noise made inside the step kernel
    def ancestral_step_(self, neg: Optional["LTXModel"], latent: torch.Tensor, video: Modality, sigma: float, sigma_up: float, sigma_down: float,
                        seed: torch.Tensor, step: int, cfg_scale: float = 1.0, denoise_mask: Optional[torch.Tensor] = None,
                        clean_latent: Optional[torch.Tensor] = None, audio_latent: Optional[torch.Tensor] = None, audio: Optional[Modality] = None,
                        audio_cfg_scale: float = 1.0, audio_denoise_mask: Optional[torch.Tensor] = None,
                        audio_clean_latent: Optional[torch.Tensor] = None) -> None:
        """In-place: one Euler-ancestral step by ONE C call (ltx2_dit_ancestral_step; with `audio_latent` / `audio` on an AudioVideo context
        ltx2_dit_ancestral_step_joint_av over both latents) -- the evaluations of guided_step_ / guided_step_joint_av_ (neg None: one, no
        guidance), then one kernel that steps to sigma_down and adds sigma_up * N(0,1) made from (seed, step, modality, element).  `seed`:
        kernels.seed_word, read on the device when the kernel runs."""
        joint = audio_latent is not None
        pos, ng = self._contexts(neg, av=joint, optional=True)
        assert seed.dtype == torch.int64 and seed.numel() == 1 and seed.is_cuda
        ngh = None if ng is None else ng._h
        if not joint:
            ts, n_ts, sg = pos._step_inputs(latent, video, sigma)
            nv.check(pos._L.ltx2_dit_ancestral_step(pos._h, ngh, nv.ptr(latent), nv.ptr(ts), n_ts, nv.ptr(sg), nv.ptr(denoise_mask), nv.ptr(clean_latent),
                                                    float(cfg_scale), float(sigma), float(sigma_up), float(sigma_down), nv.ptr(seed), int(step), nv.stream()))
            return
        ts, n_ts, sg, ats, n_ats = pos._step_inputs(latent, video, sigma, audio_latent, audio)
        nv.check(pos._L.ltx2_dit_ancestral_step_joint_av(pos._h, ngh, nv.ptr(latent), nv.ptr(audio_latent), nv.ptr(ts), n_ts, nv.ptr(ats), n_ats, nv.ptr(sg),
                                                         nv.ptr(denoise_mask), nv.ptr(clean_latent), nv.ptr(audio_denoise_mask), nv.ptr(audio_clean_latent),
                                                         float(cfg_scale), float(audio_cfg_scale), float(sigma), float(sigma_up), float(sigma_down),
                                                         nv.ptr(seed), int(step), nv.stream()))

    def capture_ancestral_graph(self, neg: Optional["LTXModel"], latent: torch.Tensor, sigmas: Sequence[float], sigma_up: Sequence[float],
                                sigma_down: Sequence[float], seed: torch.Tensor, cfg_scale: float = 1.0, denoise_mask: Optional[torch.Tensor] = None,
                                clean_latent: Optional[torch.Tensor] = None, audio_latent: Optional[torch.Tensor] = None, audio_cfg_scale: float = 1.0,
                                audio_denoise_mask: Optional[torch.Tensor] = None, audio_clean_latent: Optional[torch.Tensor] = None) -> None:
        """hipGraph-capture len(sigmas)-1 of those steps as one linear chain (ltx2_dit_graph_capture_ancestral / _joint_av): step i bakes in
        step = i, sigma_up[i] and sigma_down[i]; `seed` stays a pointer, so writing another seed into the tensor and replaying gives that
        seed's result.  The contexts are prepared first; the graph belongs to the positive context and replay_ancestral_graph() replays it."""
        joint = audio_latent is not None
        pos, ng = self._contexts(neg, av=joint, optional=True)
        n = len(sigmas) - 1
        assert len(sigma_up) == n and len(sigma_down) == n and seed.dtype == torch.int64 and seed.numel() == 1 and seed.is_cuda
        up, down = ((C.c_float * n)(*[float(v) for v in arr]) for arr in (sigma_up, sigma_down))
        if not joint:
            self._capture("ancestral", pos, ng, "ltx2_dit_graph_capture_ancestral", (latent,), sigmas, [(denoise_mask, clean_latent)], float(cfg_scale),
                          up, down, nv.ptr(seed))
        else:
            assert audio_latent.dtype == torch.float32 and audio_latent.is_contiguous()
            self._capture("ancestral", pos, ng, "ltx2_dit_graph_capture_ancestral_joint_av", (latent, audio_latent), sigmas,
                          [(denoise_mask, clean_latent), (audio_denoise_mask, audio_clean_latent)], audio_denoise_mask, audio_clean_latent,
                          float(cfg_scale), float(audio_cfg_scale), up, down, nv.ptr(seed))
        pos._graph_refs = (*pos._graph_refs, seed)

    def replay_ancestral_graph(self) -> None:
        """Replay the graph captured by capture_ancestral_graph (it belongs to the context that ran the capture)."""
        self._replay("ancestral", "no ancestral graph captured")

    # ------------------------------------------------------------------ spatio-temporal guidance on both latents (AudioVideo engine)
    def stg_step_joint_av_(self, neg: Optional["LTXModel"], latent: torch.Tensor, audio_latent: torch.Tensor, video: Modality, audio: Modality,
                           sigma: float, sigma_next: float, cfg_scale: float, audio_cfg_scale: float, stg_scale: float, audio_stg_scale: float,
                           vel_perturbed: torch.Tensor, audio_vel_perturbed: torch.Tensor, denoise_mask: Optional[torch.Tensor] = None,
                           clean_latent: Optional[torch.Tensor] = None, audio_denoise_mask: Optional[torch.Tensor] = None,
                           audio_clean_latent: Optional[torch.Tensor] = None) -> None:
        """In-place on BOTH latents, (N, C) and (Na, Ca) fp32: one Euler step of the AudioVideo model under a CFGGuider and an STGGuider per modality
        by ONE C call (ltx2_dit_stg_step_joint_av): both modalities through this context and through `neg` (None: no CFG on either), a perturbed
        forward on this context itself -- the video self-attentions of set_stg_blocks(..., 0) and the audio ones of set_stg_blocks(..., 1)
        skipped -- into vel_perturbed / audio_vel_perturbed (fp32 scratch of the latents' shapes), then x0 x 3 + both guiders +
        post_process_latent + Euler over both latents in one launch.  A modality whose STG scale is 0 is stepped as guided_step_joint_av_ steps
        it.  Both contexts are prepared by the caller (neg with the negative contexts).  There is no captured form."""
        pos, ng = self._contexts(neg, av=True, optional=True)
        ts, n_ts, sg, ats, n_ats = pos._step_inputs(latent, video, sigma, audio_latent, audio)
        for scratch in (vel_perturbed, audio_vel_perturbed):
            assert scratch.dtype == torch.float32 and scratch.is_contiguous()
        nv.check(pos._L.ltx2_dit_stg_step_joint_av(pos._h, None if ng is None else ng._h, nv.ptr(latent), nv.ptr(audio_latent), nv.ptr(ts), n_ts,
                                                   nv.ptr(ats), n_ats, nv.ptr(sg), nv.ptr(denoise_mask), nv.ptr(clean_latent),
                                                   nv.ptr(audio_denoise_mask), nv.ptr(audio_clean_latent), nv.ptr(vel_perturbed), vel_perturbed.numel(),
                                                   nv.ptr(audio_vel_perturbed), audio_vel_perturbed.numel(), float(cfg_scale), float(audio_cfg_scale),
                                                   float(stg_scale), float(audio_stg_scale), float(sigma), float(sigma_next), nv.stream()))

    # ------------------------------------------------------------------ guiders whose scalars are sums over the latent (video-only engine)
    def projected_step_(self, neg: "LTXModel", latent: torch.Tensor, video: Modality, sigma: float, sigma_next: float, mode: int, scale: float,
                        eta: float = 1.0, norm_threshold: float = 0.0, momentum: float = 0.0, first: bool = True,
                        denoise_mask: Optional[torch.Tensor] = None, clean_latent: Optional[torch.Tensor] = None) -> None:
        """In-place: latent (N, C) fp32 <- one guided Euler step under CFGStarRescalingGuider (mode 0), LtxAPGGuider (1) or
        LegacyStatefulAPGGuider (2): both evaluations as guided_step_, then the sums kernel and the projected step kernel, all enqueued by ONE C
        call (ltx2_dit_projected_step).  momentum != 0 (mode 2): the engine keeps the running guidance; `first` starts it anew."""
        pos, ng = self._contexts(neg)
        ts, n_ts, sg = pos._step_inputs(latent, video, sigma)
        nv.check(pos._L.ltx2_dit_projected_step(pos._h, ng._h, nv.ptr(latent), nv.ptr(ts), n_ts, nv.ptr(sg), nv.ptr(denoise_mask), nv.ptr(clean_latent),
                                                int(mode), float(scale), float(eta), float(norm_threshold), float(momentum), int(bool(first)),
                                                float(sigma), float(sigma_next), nv.stream()))

    def capture_projected_graph(self, neg: "LTXModel", latent: torch.Tensor, sigmas: Sequence[float], mode: int, scale: float, eta: float = 1.0,
                                norm_threshold: float = 0.0, momentum: float = 0.0, denoise_mask: Optional[torch.Tensor] = None,
                                clean_latent: Optional[torch.Tensor] = None) -> None:
        """hipGraph-capture len(sigmas)-1 projected steps over `latent` (N, C fp32) as one linear chain (ltx2_dit_graph_capture_projected); with
        momentum its head clears the running guidance, so every replay is a fresh loop.  Both contexts are prepared first (per_token=True when
        a mask is given); the graph belongs to the positive VideoOnly context and replay_projected_graph() replays it."""
        pos, ng = self._contexts(neg)
        self._capture("projected", pos, ng, "ltx2_dit_graph_capture_projected", (latent,), sigmas, [(denoise_mask, clean_latent)], int(mode),
                      float(scale), float(eta), float(norm_threshold), float(momentum))

    def replay_projected_graph(self) -> None:
        """Replay the graph captured by capture_projected_graph (it belongs to the VideoOnly context that ran the capture)."""
        self._replay("projected", "no projected graph captured")

    # ------------------------------------------------------------------ a guider per modality on both latents (AudioVideo engine)
    @staticmethod
    def _joint_guider_args(guider: dict, running: Optional[torch.Tensor], latent: torch.Tensor) -> tuple:
        """One modality's guider of the joint projected step as the C entries take it: (mode, scale, eta, norm_threshold, momentum, running).
        `guider`: mode (0 - 2 as projected_step_, 3 plain CFG, 4 not guided), scale and optionally eta, norm_threshold, momentum; `running`:
        the fp32 buffer of `latent`'s shape that mode 2 with momentum keeps its guidance in, None otherwise."""
        assert running is None or (running.dtype == torch.float32 and running.is_contiguous() and running.shape == latent.shape)
        return (int(guider["mode"]), float(guider["scale"]), float(guider.get("eta", 1.0)), float(guider.get("norm_threshold", 0.0)),
                float(guider.get("momentum", 0.0)), running)

    def projected_step_joint_av_(self, neg: "LTXModel", latent: torch.Tensor, audio_latent: torch.Tensor, video: Modality, audio: Modality, sigma: float,
                                 sigma_next: float, video_guider: dict, audio_guider: dict, first: bool = True,
                                 running: Optional[torch.Tensor] = None, audio_running: Optional[torch.Tensor] = None,
                                 denoise_mask: Optional[torch.Tensor] = None, clean_latent: Optional[torch.Tensor] = None,
                                 audio_denoise_mask: Optional[torch.Tensor] = None, audio_clean_latent: Optional[torch.Tensor] = None) -> None:
        """In-place on BOTH latents, (N, C) and (Na, Ca) fp32: one guided Euler step of the AudioVideo model with a guider per modality by ONE C
        call (ltx2_dit_projected_step_joint_av): both modalities through this context and through `neg`, then one sums launch over the
        modalities whose guider reads sums and one step launch over both latents.  video_guider / audio_guider: dict(mode, scale[, eta,
        norm_threshold, momentum]) as pipelines.common.projected_guider_args gives it, mode 3 for a plain CFGGuider, mode 4 for none.
        running / audio_running: the buffer a mode-2 guider with momentum keeps its guidance in; `first` starts it anew."""
        pos, ng = self._contexts(neg, av=True)
        ts, n_ts, sg, ats, n_ats = pos._step_inputs(latent, video, sigma, audio_latent, audio)
        per = [x for *g, run in (self._joint_guider_args(video_guider, running, latent), self._joint_guider_args(audio_guider, audio_running, audio_latent))
               for x in (*g, nv.ptr(run), 0 if run is None else run.numel())]
        nv.check(pos._L.ltx2_dit_projected_step_joint_av(pos._h, ng._h, nv.ptr(latent), nv.ptr(audio_latent), nv.ptr(ts), n_ts, nv.ptr(ats), n_ats,
                                                         nv.ptr(sg), nv.ptr(denoise_mask), nv.ptr(clean_latent), nv.ptr(audio_denoise_mask),
                                                         nv.ptr(audio_clean_latent), *per, int(bool(first)), float(sigma), float(sigma_next),
                                                         nv.stream()))

    def capture_projected_joint_graph(self, neg: "LTXModel", latent: torch.Tensor, audio_latent: torch.Tensor, sigmas: Sequence[float],
                                      video_guider: dict, audio_guider: dict, running: Optional[torch.Tensor] = None,
                                      audio_running: Optional[torch.Tensor] = None, denoise_mask: Optional[torch.Tensor] = None,
                                      clean_latent: Optional[torch.Tensor] = None, audio_denoise_mask: Optional[torch.Tensor] = None,
                                      audio_clean_latent: Optional[torch.Tensor] = None) -> None:
        """hipGraph-capture len(sigmas)-1 of those steps over both latents, updated in place on replay
        (ltx2_dit_graph_capture_projected_joint_av); its head clears each running buffer, so every replay is a fresh loop.  Both contexts are
        prepared first (per_token=True when a mask is given); the graph belongs to this context and replay_projected_joint_graph() replays it.
        The tensors must stay alive while it is replayed."""
        pos, ng = self._contexts(neg, av=True)
        assert audio_latent.dtype == torch.float32 and audio_latent.is_contiguous()
        self._capture("projected_joint", pos, ng, "ltx2_dit_graph_capture_projected_joint_av", (latent, audio_latent), sigmas,
                      [(denoise_mask, clean_latent), (audio_denoise_mask, audio_clean_latent)], audio_denoise_mask, audio_clean_latent,
                      *self._joint_guider_args(video_guider, running, latent), *self._joint_guider_args(audio_guider, audio_running, audio_latent))

    def replay_projected_joint_graph(self) -> None:
        """Replay the graph captured by capture_projected_joint_graph."""
        self._replay("projected_joint", "no joint projected graph captured")

    # ------------------------------------------------------------------ res_2s second-order sampling (video-only engine)
    def res2s_step_(self, neg: Optional["LTXModel"], latent: torch.Tensor, video: Modality, video_sub: Optional[Modality], sigma: float,
                    sigma_next: float, cfg_scale: float, denoise_mask: Optional[torch.Tensor] = None,
                    clean_latent: Optional[torch.Tensor] = None) -> None:
        """In-place: latent (N, C) fp32 <- one res_2s step (reference pipelines/ti2vid_hq.py:185-273) by ONE C call (ltx2_dit_res2s_step):
        forward(self) and forward(neg) at `video`'s timesteps, the midpoint kernel, both again from the midpoint latent at `video_sub`'s
        timesteps (those of the sub-sigma sqrt(sigma * sigma_next)), the combine kernel.  neg None: no guidance.  video_sub may be None
        only for the final step (sigma_next <= 0.001), which is one pair of evaluations and latent = d.  Both contexts are prepared by the
        caller (neg with the negative context)."""
        pos, ng = self._contexts(neg, optional=True)
        ts, n_ts, sg = pos._step_inputs(latent, video, sigma)
        ts_sub = sg_sub = None
        if video_sub is not None:
            ts_sub, n_sub = pos._timesteps(video_sub)
            assert n_sub == n_ts, "both evaluations take one timestep, or one per token"
            if pos.cross_attention_adaln:
                sg_sub = pos._sigma(video_sub)
        nv.check(pos._L.ltx2_dit_res2s_step(pos._h, None if ng is None else ng._h, nv.ptr(latent), nv.ptr(ts), n_ts, nv.ptr(sg), nv.ptr(ts_sub),
                                            nv.ptr(sg_sub), nv.ptr(denoise_mask), nv.ptr(clean_latent), float(cfg_scale), float(sigma),
                                            float(sigma_next), nv.stream()))

    def capture_res2s_graph(self, neg: Optional["LTXModel"], latent: torch.Tensor, sigmas: Sequence[float], cfg_scale: float,
                            denoise_mask: Optional[torch.Tensor] = None, clean_latent: Optional[torch.Tensor] = None) -> None:
        """hipGraph-capture len(sigmas)-1 res_2s steps over `latent` (N, C fp32) as one linear chain (ltx2_dit_graph_capture_res2s).  Both
        contexts are prepared first (per_token=True when a mask is given); the graph belongs to the positive VideoOnly context and
        replay_res2s_graph() replays it.  The tensors must stay alive while it is replayed."""
        pos, ng = self._contexts(neg, optional=True)
        self._capture("res2s", pos, ng, "ltx2_dit_graph_capture_res2s", (latent,), sigmas, [(denoise_mask, clean_latent)], float(cfg_scale))

    def replay_res2s_graph(self) -> None:
        """Replay the graph captured by capture_res2s_graph (it belongs to the VideoOnly context that ran the capture)."""
        self._replay("res2s", "no res_2s graph captured")

    # ------------------------------------------------------------------ joint audio+video res_2s sampling (AudioVideo engine)
    def res2s_step_av_(self, neg: Optional["LTXModel"], latent: torch.Tensor, audio_latent: torch.Tensor, video: Modality, audio: Modality,
                       video_sub: Optional[Modality], audio_sub: Optional[Modality], sigma: float, sigma_next: float, cfg_scale: float,
                       audio_cfg_scale: float, denoise_mask: Optional[torch.Tensor] = None, clean_latent: Optional[torch.Tensor] = None,
                       audio_denoise_mask: Optional[torch.Tensor] = None, audio_clean_latent: Optional[torch.Tensor] = None) -> None:
        """In-place on BOTH latents, (N, C) and (Na, Ca) fp32: one joint res_2s step (reference pipelines/ti2vid_hq.py:153-319) by ONE C call
        (ltx2_dit_res2s_step_av): both modalities through this context and through `neg` at `video` / `audio`'s timesteps, the midpoint
        kernel over both latents in one launch, both contexts again from the midpoint latents at `video_sub` / `audio_sub`'s timesteps
        (those of the sub-sigma sqrt(sigma * sigma_next)), the combine kernel likewise.  The video is guided by cfg_scale, the audio by
        audio_cfg_scale; neg None: no guidance.  The sub modalities may be None only for the final step (sigma_next <= 0.001).  Both
        contexts are prepared by the caller (neg with the negative contexts)."""
        pos, ng = self._contexts(neg, av=True, optional=True)
        assert (video_sub is None) == (audio_sub is None), "video_sub and audio_sub go together (both None: the final step)"
        ts, n_ts, sg, ats, n_ats = pos._step_inputs(latent, video, sigma, audio_latent, audio)
        ts_sub = ats_sub = sg_sub = None
        if video_sub is not None:
            ts_sub, n_sub = pos._timesteps(video_sub)
            ats_sub, n_asub = pos._timesteps(audio_sub)
            assert n_sub == n_ts and n_asub == n_ats, "both evaluations take one timestep, or one per token"
            sg_sub = pos._sigma(video_sub)
        nv.check(pos._L.ltx2_dit_res2s_step_av(pos._h, None if ng is None else ng._h, nv.ptr(latent), nv.ptr(audio_latent), nv.ptr(ts), n_ts,
                                               nv.ptr(ats), n_ats, nv.ptr(sg), nv.ptr(ts_sub), nv.ptr(ats_sub), nv.ptr(sg_sub), nv.ptr(denoise_mask),
                                               nv.ptr(clean_latent), nv.ptr(audio_denoise_mask), nv.ptr(audio_clean_latent), float(cfg_scale),
                                               float(audio_cfg_scale), float(sigma), float(sigma_next), nv.stream()))

    # ------------------------------------------------------------------ Heun sampling and the GE velocity correction (OneStagePipeline)
    def heun_step_(self, neg: Optional["LTXModel"], latent: torch.Tensor, video: Modality, video_next: Optional[Modality], sigma: float,
                   sigma_next: float, cfg_scale: float, ge_gamma: float = 0.0, first: bool = True, denoise_mask: Optional[torch.Tensor] = None,
                   clean_latent: Optional[torch.Tensor] = None) -> None:
        """In-place: latent (N, C) fp32 <- one Heun step (reference pipelines/one_stage.py:366-459 under a CFGGuider) by ONE C call
        (ltx2_dit_heun_step): forward(self) and forward(neg) at `video`'s timesteps, the predictor kernel, both again from the predicted
        latent at `video_next`'s timesteps (those of sigma_next), the corrector kernel.  neg None: no guidance.  video_next may be None only
        when sigma_next == 0, which is one pair of evaluations and latent = d.  ge_gamma > 0: the GE velocity correction, its state kept by
        the engine; `first` starts it anew.  Both contexts are prepared by the caller (neg with the negative context)."""
        pos, ng = self._contexts(neg, optional=True)
        ts, n_ts, sg = pos._step_inputs(latent, video, sigma)
        ts_next = sg_next = None
        if video_next is not None:
            ts_next, n_next = pos._timesteps(video_next)
            assert n_next == n_ts, "both evaluations take one timestep, or one per token"
            if pos.cross_attention_adaln:
                sg_next = pos._sigma(video_next)
        nv.check(pos._L.ltx2_dit_heun_step(pos._h, None if ng is None else ng._h, nv.ptr(latent), nv.ptr(ts), n_ts, nv.ptr(sg), nv.ptr(ts_next),
                                           nv.ptr(sg_next), nv.ptr(denoise_mask), nv.ptr(clean_latent), float(cfg_scale), float(ge_gamma),
                                           int(bool(first)), float(sigma), float(sigma_next), nv.stream()))

    def capture_heun_graph(self, neg: Optional["LTXModel"], latent: torch.Tensor, sigmas: Sequence[float], cfg_scale: float, ge_gamma: float = 0.0,
                           denoise_mask: Optional[torch.Tensor] = None, clean_latent: Optional[torch.Tensor] = None) -> None:
        """hipGraph-capture len(sigmas)-1 Heun steps over `latent` (N, C fp32) as one linear chain (ltx2_dit_graph_capture_heun); with GE its
        head clears the kept velocity, so every replay is a fresh loop.  Both contexts are prepared first (per_token=True when a mask is
        given); the graph belongs to the positive VideoOnly context and replay_heun_graph() replays it."""
        pos, ng = self._contexts(neg, optional=True)
        self._capture("heun", pos, ng, "ltx2_dit_graph_capture_heun", (latent,), sigmas, [(denoise_mask, clean_latent)], float(cfg_scale), float(ge_gamma))

    def replay_heun_graph(self) -> None:
        """Replay the graph captured by capture_heun_graph (it belongs to the VideoOnly context that ran the capture)."""
        self._replay("heun", "no Heun graph captured")

    def heun_step_av_(self, neg: Optional["LTXModel"], latent: torch.Tensor, audio_latent: torch.Tensor, video: Modality, audio: Modality,
                      video_next: Optional[Modality], audio_next: Optional[Modality], sigma: float, sigma_next: float, cfg_scale: float,
                      audio_cfg_scale: float, ge_gamma: float = 0.0, first: bool = True, denoise_mask: Optional[torch.Tensor] = None,
                      clean_latent: Optional[torch.Tensor] = None, audio_denoise_mask: Optional[torch.Tensor] = None,
                      audio_clean_latent: Optional[torch.Tensor] = None) -> None:
        """In-place on BOTH latents, (N, C) and (Na, Ca) fp32: one joint Heun step (reference pipelines/one_stage.py:600-724) by ONE C call
        (ltx2_dit_heun_step_av): each kernel one launch over both latents, the video under cfg_scale and the audio under audio_cfg_scale,
        GE on the video alone.  The *_next modalities may be None only when sigma_next == 0."""
        pos, ng = self._contexts(neg, av=True, optional=True)
        assert (video_next is None) == (audio_next is None), "video_next and audio_next go together (both None: sigma_next == 0)"
        ts, n_ts, sg, ats, n_ats = pos._step_inputs(latent, video, sigma, audio_latent, audio)
        ts_next = ats_next = sg_next = None
        if video_next is not None:
            ts_next, n_next = pos._timesteps(video_next)
            ats_next, n_anext = pos._timesteps(audio_next)
            assert n_next == n_ts and n_anext == n_ats, "both evaluations take one timestep, or one per token"
            sg_next = pos._sigma(video_next)
        nv.check(pos._L.ltx2_dit_heun_step_av(pos._h, None if ng is None else ng._h, nv.ptr(latent), nv.ptr(audio_latent), nv.ptr(ts), n_ts,
                                              nv.ptr(ats), n_ats, nv.ptr(sg), nv.ptr(ts_next), nv.ptr(ats_next), nv.ptr(sg_next), nv.ptr(denoise_mask),
                                              nv.ptr(clean_latent), nv.ptr(audio_denoise_mask), nv.ptr(audio_clean_latent), float(cfg_scale),
                                              float(audio_cfg_scale), float(ge_gamma), int(bool(first)), float(sigma), float(sigma_next), nv.stream()))

    def ge_step_(self, neg: Optional["LTXModel"], latent: torch.Tensor, video: Modality, sigma: float, sigma_next: float, cfg_scale: float,
                 ge_gamma: float, first: bool = True, denoise_mask: Optional[torch.Tensor] = None, clean_latent: Optional[torch.Tensor] = None) -> None:
        """In-place: latent (N, C) fp32 <- one Euler step with the GE velocity correction (reference pipelines/one_stage.py:267-326 under a
        CFGGuider; neg None: no guidance) by ONE C call (ltx2_dit_ge_step).  The engine keeps the previous step's velocity; `first` starts it
        anew."""
        pos, ng = self._contexts(neg, optional=True)
        ts, n_ts, sg = pos._step_inputs(latent, video, sigma)
        nv.check(pos._L.ltx2_dit_ge_step(pos._h, None if ng is None else ng._h, nv.ptr(latent), nv.ptr(ts), n_ts, nv.ptr(sg), nv.ptr(denoise_mask),
                                         nv.ptr(clean_latent), float(cfg_scale), float(ge_gamma), int(bool(first)), float(sigma), float(sigma_next),
                                         nv.stream()))

    # ------------------------------------------------------------------ multi-modal guidance: CFG + STG + modality isolation (AudioVideo engine)
    def forward_isolated(self, video: Modality, audio: Modality) -> Tuple[torch.Tensor, torch.Tensor]:
        """The modality-isolated forward (ltx2_dit_forward_isolated_av; the reference's SKIP_A2V_CROSS_ATTN + SKIP_V2A_CROSS_ATTN over every
        block, pipelines/two_stage.py:356-364): __call__(video, audio) with no cross-modal attention in any layer, so each modality's
        velocity depends on its own latent alone.  -> (video velocity (1, N, C), audio velocity (1, Na, Ca)).  AudioVideo models only."""
        if not self.is_av:
            raise ValueError("forward_isolated runs on an AudioVideo model (a VideoOnly model has no cross-modal attention to skip)")
        if audio is None:
            raise ValueError("forward_isolated needs the audio modality")
        self._check_inputs(video, audio, None)
        ts, n_ts = self._timesteps(video)
        ats, n_ats = self._timesteps(audio)
        self._ensure_prepared(video, per_token=(n_ts != 1 or n_ats != 1), audio=audio)
        self._apply_context_masks(video, audio)
        lat = video.latent[0].to(self.device, torch.float32).contiguous()
        alat = audio.latent[0].to(self.device, torch.float32).contiguous()
        out = torch.empty(lat.shape[0], self.out_channels, device=self.device, dtype=torch.float32)
        aout = torch.empty(alat.shape[0], self.AUDIO_OUT_CHANNELS, device=self.device, dtype=torch.float32)
        vs, as_ = self._sigma(video), self._sigma(audio)
        nv.check(self._L.ltx2_dit_forward_isolated_av(self._h, nv.ptr(lat), nv.ptr(ts), n_ts, nv.ptr(vs), nv.ptr(alat), nv.ptr(ats), n_ats, nv.ptr(as_),
                                                      nv.ptr(out), nv.ptr(aout), nv.stream()))
        return out[None], aout[None]

    def mm_guided_step_av_(self, neg: Optional["LTXModel"], latent: torch.Tensor, audio_latent: torch.Tensor, video: Modality, audio: Modality,
                           sigma: float, sigma_next: float, video_params, audio_params, isolated: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                           perturbed: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, denoise_mask: Optional[torch.Tensor] = None,
                           clean_latent: Optional[torch.Tensor] = None, audio_denoise_mask: Optional[torch.Tensor] = None,
                           audio_clean_latent: Optional[torch.Tensor] = None) -> None:
        """In-place on BOTH latents, (N, C) and (Na, Ca) fp32: one step of the two-stage pipeline's stage 1 (reference
        pipelines/two_stage.py:314-401) by ONE C call (ltx2_dit_mm_guided_step_av): both modalities through this context, through `neg` (None:
        no CFG term), through this context with the self-attentions of set_stg_blocks skipped into the `perturbed` scratch pair (None: no
        STG term) and with every cross-modal attention skipped into the `isolated` pair (None: no modality term); then
        MultiModalGuider.calculate with video_params / audio_params (MultiModalGuiderParams), post_process_latent and the Euler step of both
        latents -- one launch, or per modality a sums and a step launch where rescale_scale != 0.  A scratch pair is (video (N, C), audio
        (Na, Ca)) fp32.  Both contexts are prepared by the caller (neg with the negative contexts)."""
        pos, ng = self._contexts(neg, av=True, optional=True)
        ts, n_ts, sg, ats, n_ats = pos._step_inputs(latent, video, sigma, audio_latent, audio)
        bufs = []
        for pair in (isolated, perturbed):
            for t in (pair or (None, None)):
                assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
                bufs += [nv.ptr(t), 0 if t is None else t.numel()]
        scales = [float(s) for p in (video_params, audio_params) for s in (p.cfg_scale, p.stg_scale, p.modality_scale, p.rescale_scale)]
        nv.check(pos._L.ltx2_dit_mm_guided_step_av(pos._h, None if ng is None else ng._h, nv.ptr(latent), nv.ptr(audio_latent), nv.ptr(ts), n_ts,
                                                   nv.ptr(ats), n_ats, nv.ptr(sg), nv.ptr(denoise_mask), nv.ptr(clean_latent), nv.ptr(audio_denoise_mask),
                                                   nv.ptr(audio_clean_latent), *bufs, *scales, float(sigma), float(sigma_next), nv.stream()))

    def replace_weights(self, tensors: Dict[str, torch.Tensor]) -> None:
        """Re-register engine-layout tensors (names of weight_tensors()) in place of the ones held now -- the HQ pipeline's LoRA fusion for
        its second stage and the restore after it.  Contexts built over the old tensors (video twin, clone) are rebuilt on demand."""
        for k, v in tensors.items():
            if k not in self._w or self._w[k].shape != v.shape or self._w[k].dtype != v.dtype:
                raise ValueError(f"{k}: not a registered weight of this shape and dtype")
            self._register(k, v)
        self._prep_key = None
        self._twin = None
        self._clone = None

    def replay_denoise_graph(self) -> None:
        nv.check(self._L.ltx2_dit_graph_launch(self._h, nv.stream()))

    # ------------------------------------------------------------------ measurement
    def profile_begin(self, epilogue: int = -1) -> None:
        """HIP-event bracket every launch of one GEMM kernel instantiation (or all, -1)."""
        nv.check(self._L.ltx2_dit_profile_begin(self._h, epilogue))

    def profile_end(self) -> Tuple[float, int, float]:
        """-> (summed kernel ms, launches, 2*M*N*K flops) since profile_begin."""
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        nv.check(self._L.ltx2_dit_profile_end(self._h, C.byref(ms), C.byref(n), C.byref(fl)))
        return ms.value, n.value, fl.value


class X0Model:
    """x0 = latent - timesteps * velocity per modality (reference model.py:884-936)."""

    def __init__(self, velocity_model: LTXModel):
        self.velocity_model = velocity_model

    @staticmethod
    def _denoise(m: Modality, v: torch.Tensor) -> torch.Tensor:
        lat = m.latent[0].to(v.device, torch.float32).contiguous()
        ts = m.timesteps.to(v.device, torch.float32).reshape(-1)
        return K.x0_from_velocity(lat, v[0], ts)[None]

    def __call__(self, video: Optional[Modality] = None, audio: Optional[Modality] = None, perturbations=None):
        out = self.velocity_model(video, audio, perturbations=perturbations)
        if isinstance(out, tuple):
            if out[1].shape[1] == 0:            # video-only inference on an AudioVideo model: nothing to denoise on the audio side
                return self._denoise(video, out[0]), out[1]
            return self._denoise(video, out[0]), self._denoise(audio, out[1])
        return self._denoise(video, out)

    def forward_isolated(self, video: Modality, audio: Modality) -> Tuple[torch.Tensor, torch.Tensor]:
        """x0 of both modalities from LTXModel.forward_isolated (no cross-modal attention in any layer)."""
        v, a = self.velocity_model.forward_isolated(video, audio)
        return self._denoise(video, v), self._denoise(audio, a)


# aliases kept by the reference for backward compatibility (model.py:939-941)
LTXAVModel = LTXModel
X0AVModel = X0Model
