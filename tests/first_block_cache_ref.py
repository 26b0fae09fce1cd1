"""fp32 torch / float64 numpy restatement (CPU) of the first-block cache: the metric, the decision, the slot state, the driver's forced first and
last steps, and the loops, over the oracle's DiT run block by block from its public pieces.  Written from the definition (DESIGN.md section 1,
include/ltx2hip.h).  Checker side only: nothing here is imported by the package."""
import numpy as np
import torch
import torch.nn.functional as F

import standard_cfg_ref as R
from oracle import dit


def metric64(r, head_prev):
    """(num, den) = (sum |r - head_prev|, sum |head_prev|) over all elements, in float64."""
    r, p = np.asarray(r, np.float64), np.asarray(head_prev, np.float64)
    return float(np.abs(r - p).sum()), float(np.abs(p).sum())


def decide(num, den, t):
    """Skip iff num < t*den, t rounded to float32 as the engine takes it; no division; den == 0 and t == 0 never skip."""
    t = float(np.float32(t))
    return bool(t > 0 and den > 0 and num < t * den)


class Slot:
    def __init__(self):
        self.head_prev, self.tail, self.valid, self.force = None, None, False, False
        self.evaluations = self.skips = 0
        self.log = []           # per evaluation: (skipped, num, den) -- num / den None where no metric was formed (invalid slot)


class FirstBlockCache:
    """threshold t and n_slots slots.  evaluate(slot, h0, head, tail) -> the residual stream in front of the output head, where head(h0) runs block 0
    and tail(h1) blocks 1..L-1."""

    def __init__(self, threshold, n_slots):
        if not threshold >= 0:
            raise ValueError("threshold must be >= 0")
        self.t, self.slots = threshold, [Slot() for _ in range(n_slots)]

    def reset(self):
        self.slots = [Slot() for _ in self.slots]

    def force_next(self, slot=-1):
        for k, s in enumerate(self.slots):
            if slot < 0 or slot == k:
                s.force = True

    def evaluate(self, slot, h0, head, tail):
        s = self.slots[slot]
        h1 = head(h0)
        r = h1 - h0                                     # fp32, element-wise
        forced, s.force = s.force, False
        s.evaluations += 1
        num = den = None
        if s.valid:
            num, den = metric64(r.numpy(), s.head_prev.numpy())
            if not forced and decide(num, den, self.t):
                s.skips += 1
                s.log.append((True, num, den))
                return h1 + s.tail                      # head_prev and tail stay as they are
        hL = tail(h1)
        s.tail, s.head_prev, s.valid = hL - h1, r, True
        s.log.append((False, num, den))
        return hL

    def stats(self):
        return [dict(evaluations=s.evaluations, skips=s.skips) for s in self.slots]

    def pattern(self, slot=0):
        return [e[0] for e in self.slots[slot].log]


class BlockwiseDiT:
    """oracle.dit.velocity_model cut into embed / blocks / output head, for one prompt and one token grid."""

    def __init__(self, cfg, w, context, positions):
        self.cfg, self.w = cfg, w
        ctx = context.float()
        if cfg.caption_channels is not None:
            ctx = dit.caption_projection(ctx, w)
        self.ctx = ctx.reshape(context.shape[0], -1, cfg.inner_dim)
        self.pe = dit.rope_split_tables(positions.float(), cfg.inner_dim, cfg.num_attention_heads, cfg.positional_embedding_theta,
                                        cfg.positional_embedding_max_pos)

    def blocks(self, x, emb, first, last):
        for i in range(first, last):
            x = dit.transformer_block(x, self.ctx, emb, self.pe, self.w, i, self.cfg, None)
        return x

    def velocity(self, latent, timesteps, cache=None, slot=0):
        cfg, w, b = self.cfg, self.w, latent.shape[0]
        h0 = dit.linear(latent.float(), w, "patchify_proj")
        emb, e = dit.prepare_timestep(timesteps.reshape(b, -1), w, cfg, b)
        if cache is None:
            x = self.blocks(h0, emb, 0, cfg.num_layers)
        else:
            x = cache.evaluate(slot, h0, lambda h: self.blocks(h, emb, 0, 1), lambda h: self.blocks(h, emb, 1, cfg.num_layers))
        ss = w["scale_shift_table"].float()[None, None, :, :] + e[:, :, None, :]
        x = F.layer_norm(x, (cfg.inner_dim,), eps=cfg.norm_eps)
        return dit.linear(x * (1 + ss[:, :, 1]) + ss[:, :, 0], w, "proj_out")


def cached_loop(tokens, sigmas, cache, pos_model, neg_model=None, cfg_scale=1.0, guidance_rescale=0.0):
    """The standard loop on (1, N, C) tokens with the cache on, the driver's rules included: reset at the start, the last step forced (the first
    computes anyway: its slots are not valid).  neg_model None: the plain loop through slot 0; otherwise the guided one, the positive pass in slot 0
    and the negative one in slot 1, the step as standard_cfg_ref states it."""
    x = tokens.float()
    n = len(sigmas) - 1
    cache.reset()
    for i in range(n):
        if i == n - 1:
            cache.force_next(-1)
        s = float(sigmas[i])
        ts = torch.tensor([s])
        cond = x - ts[:, None, None] * pos_model.velocity(x, ts, cache, 0)
        if neg_model is None:
            g = cond
        else:
            uncond = x - ts[:, None, None] * neg_model.velocity(x, ts, cache, 1)
            g = uncond + cfg_scale * (cond - uncond)
            if guidance_rescale > 0:
                stats = torch.from_numpy(R.channel_stats64(g[0].numpy(), cond[0].numpy())).float()
                g = R.rescale_noise_cfg(g[0], cond[0], stats, guidance_rescale)[None]
        x = R.euler_x0(x, g, s, float(sigmas[i + 1]))
    return x
