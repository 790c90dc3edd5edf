"""eps-model of the DDIM loops (rows X2 / G1 of SURVEY.md section 8a): a from-scratch Stable-Diffusion-2.1-base-shaped
conditional UNet in plain torch, used as the `eps_model(latents, t, ctx)` callable of ddim.py.

Why it exists: the reference delegates this to diffusers==0.26.0 `UNet2DConditionModel` + HF weights
`stabilityai/stable-diffusion-2-1-base` (extract.py:56-60,66-69), neither of which is available here (no network).  The
architecture below follows the published SD 2.1-base `unet/config.json` (block_out_channels 320/640/1280/1280,
2 resnets per block, 1 transformer layer per attention block, heads 5/10/20/20 x 64, cross_attention_dim 1024, linear
projections, GEGLU feed-forward, 32-group GroupNorm) and keeps diffusers' parameter names, so a diffusers-layout
safetensors state dict loads 1:1 (`load_diffusers_state_dict`).  Without a weight directory the weights are seeded
synthetic -- throughput is representative, image content is not.

On the GPU (fp16 / bf16) every convolution, linear layer and attention runs on the hand-written MFMA kernels of libgswm (PF implicit-GEMM
convolutions, the gsw_gemm matmul engine, the flash-attention kernel); the plain torch ops remain for CPU / meta tensors (FLOP counting,
CPU baseline) and are counted in `FALLBACKS` when a GPU call has to use them.
"""
from __future__ import annotations

import math
import os
import warnings
from typing import Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as N
from . import checkpoint, codec, graph, pf, xattn


# Fused HIP elementwise kernels (libgswm: gsw_groupnorm_silu, gsw_geglu) replace torch's GroupNorm -> SiLU (-> broadcast add)
# and GELU -> mul chains on the GPU; the plain torch ops remain for CPU / meta tensors (FLOP counting, CPU baseline).
FUSED_KERNELS = True


def _fusable(x: torch.Tensor) -> bool:
    return FUSED_KERNELS and x.is_cuda and x.dtype in (torch.float16, torch.bfloat16, torch.float32) and x.is_contiguous() \
        and (x.shape[-1] * x.shape[-2]) % 8 == 0


def gn_act(x: torch.Tensor, norm: nn.GroupNorm, act: bool = True, pre_bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(GroupNorm(x + pre_bias[:, :, None, None]))"""
    if _fusable(x):
        return codec.groupnorm_silu(x, norm.weight, norm.bias, norm.num_groups, norm.eps, act=act, pre_bias=pre_bias)
    if pre_bias is not None:
        x = x + pre_bias[:, :, None, None]
    y = norm(x)
    return F.silu(y) if act else y


# Padded-flat NHWC path: every 3x3 / 1x1 / stride-2 convolution of the UNet runs as a hand-written MFMA implicit GEMM (the matmul engine of
# csrc/gswm_mm.hip through csrc/gswm_conv.hip; conv_in / conv_out's 4-channel side padded to one 64-wide tile) with bias, time-embedding and
# residual adds fused into its epilogue, GroupNorm+SiLU as the PF kernels, Upsample2D as four sub-pixel launches; the transformer blocks run on
# the same engine (OWN_GEMM) and the flash-attention kernel (OWN_ATTENTION).
USE_PF = True


def _pw(conv: nn.Conv2d) -> torch.Tensor:
    return pf.cached(conv, "_gsw_packed", (conv.weight,), lambda: pf.pack_conv_weight(conv.weight.detach()))


UPSAMPLE_SUBPIXEL = True   # Upsample2D = four 2x2 convolutions of the low-resolution tensor (gsw_conv_up2x_pf) instead of upsample + 3x3

CACHE_CONTEXT_KV = True   # cross-attention K / V^T of a context tensor are computed once and reused across the steps of a loop

FUSED_QK = True       # self-attention: q and k projections as one GEMM (own attention kernel reads them as column slices)

FUSED_QKV = False     # ... and the transposed value projection from the same launch (gsw_gemm_qkv: the tokens are read once).  Measured: no gain --
                      # forward 113.6 vs 113.3 ms at 128 rows, 60.5 vs 60.2 at 64 (the value part loses the 12-wave form, the launch runs at 235 registers);
                      # kept as an A/B switch, bit-identical to the two launches (tests/test_gpu_qkv.py)

OWN_ATTENTION = True  # attention with head_dim 40 / 64 / 80 / 160, any query count, keys % 8 == 0 runs on gsw_attention instead of torch SDPA

OWN_GEMM = True       # every dense linear layer (q / k / v / out projections, proj_in / proj_out, feed-forward, time embedding) on the
                      # hand-written matmul engine (gsw_gemm, csrc/gswm_mm.hip) with bias / residual / GEGLU / V^T epilogues fused in

FOLD_FF_OUT = os.environ.get("GSW_FOLD_FF_OUT", "1") != "0"      # Transformer2DModel: the last block's ff.net[2] folded into proj_out -- one two-segment GEMM
                      # [h | x] [Wp W2 | Wp]^T + (Wp b2 + bp) scattered into the PF tensor instead of two launches with the stream between them written and re-read
                      # (pf.gemm2 / gsw_gemm2_ex; engine path only: the small-batch kernel keeps the two launches).  0 = the two launches (A/B)

FALLBACKS = {}        # (reason -> count) of GPU half-precision calls that left the hand-written path; bench and the full-size tests assert it stays empty

# Leaving the hand-written path (a shape off the engine's K % 64 / N % 8 grid, attention keys % 8, a lattice the padded-flat layout does not take) RAISES by default: a
# 200 x 136 image must not silently run a different backend (hipBLASLt / MIOpen / aotriton).  GSW_STRICT_KERNELS=0, `--strict_kernels 0` of the harness or
# `unet.STRICT = vae.STRICT = False` opt into the library kernels; every such call is then counted in FALLBACKS and warned about once per reason.
STRICT = os.environ.get("GSW_STRICT_KERNELS", "1") != "0"


def _note_fallback(why: str):
    if STRICT:
        raise RuntimeError("gswm unet (strict kernels): " + why + " -- this call would run a library kernel (hipBLASLt / MIOpen / SDPA); "
                           "pass --strict_kernels 0 to allow it")
    if why not in FALLBACKS:       # loud, once per reason: a GPU run that leaves the hand-written kernels should never be silent
        warnings.warn("gswm unet: " + why, RuntimeWarning, stacklevel=3)
    FALLBACKS[why] = FALLBACKS.get(why, 0) + 1


def _own_gemm_ok(x: torch.Tensor, K: int, N: int) -> bool:
    """The matmul engine takes fp16 / bf16 device tensors with K % 64 == 0 and N % 8 == 0 (every SD 1.x / 2.x linear)."""
    if not (OWN_GEMM and USE_PF and FUSED_KERNELS and pf.half_gpu(x)):
        return False
    if K % 64 or N % 8:
        _note_fallback(f"linear K={K} N={N}: library GEMM")
        return False
    return True


def _wb(lin: nn.Linear, x: torch.Tensor):
    """(weight, bias) of a linear layer as the engine wants them: contiguous, the activations' dtype (a fp32 parameter under an fp16
    activation must not be read as fp16 bytes)."""
    if lin.weight.dtype != x.dtype or lin.weight.device != x.device or not lin.weight.is_contiguous():
        raise ValueError(f"linear weight is {lin.weight.dtype} on {lin.weight.device}, activations are {x.dtype} on {x.device}")
    return lin.weight, lin.bias


def _lin(x: torch.Tensor, lin: nn.Linear, resid: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, rowstats: bool = False) -> torch.Tensor:
    """Linear (+ residual in the epilogue) on the matmul engine, else torch.  out: written in place (same shape, contiguous).
    rowstats: the launch also leaves the row records a following LayerNorm can be folded from (pf.ln_stat) on the result."""
    if _own_gemm_ok(x, lin.in_features, lin.out_features):
        w, b = _wb(lin, x)
        return pf.gemm(x.contiguous(), w, b, resid=None if resid is None else resid.contiguous(), out=out, rowstats=rowstats)
    y = lin(x)
    y = y if resid is None else y + resid
    return y if out is None else out.copy_(y)


def _lin_t(x: torch.Tensor, lin: nn.Linear, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B, S, K] -> (lin(x))^T = [B, N, S]: the value projection in the layout the attention kernel consumes."""
    b, n, _ = x.shape
    if _own_gemm_ok(x, lin.in_features, lin.out_features) and n % 8 == 0:
        w, bias = _wb(lin, x)
        return pf.gemm(x.contiguous(), w, bias, mode="trans", tokens=n, out=out)
    vt = torch.bmm(lin.weight.unsqueeze(0).expand(b, -1, -1), x.transpose(1, 2))
    vt = vt if lin.bias is None else vt + lin.bias[None, :, None]
    return vt if out is None else out.copy_(vt)


def timestep_embedding(t: torch.Tensor, dim: int, max_period: float = 10000.0) -> torch.Tensor:
    """Sinusoidal embedding, flip_sin_to_cos=True, freq_shift=0 (SD config): [cos | sin]."""
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float32, device=t.device) / half)
    args = t.float()[:, None] * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


class TimestepEmbedding(nn.Module):
    def __init__(self, in_dim, dim):
        super().__init__()
        self.linear_1 = nn.Linear(in_dim, dim)
        self.linear_2 = nn.Linear(dim, dim)

    def forward(self, x):
        return _lin(F.silu(_lin(x, self.linear_1)), self.linear_2)


class TembRows:
    """silu(time embedding) [B, temb] and, per resnet, its time_emb_proj output as a column slice [B, cout] of ONE GEMM over the concatenated
    projection weights (22 resnets -> one launch instead of 22; the convolution epilogue reads the slice through its row stride)."""
    __slots__ = ("act", "rows", "table", "widths")

    def __init__(self, act, table, widths):
        """table: the [B, sum of channels] matrix; widths: (key, channels) per resnet in column order (key: id(resnet)) -> rows[key] = its column slice"""
        self.act, self.table, self.widths, self.rows, off = act, table, widths, {}, 0
        for key, n in widths:
            self.rows[key] = table[:, off:off + n]
            off += n

    def doubled(self) -> "TembRows":
        """the rows of B images -> of the 2B images of the doubled batch"""
        return TembRows(None if self.act is None else torch.cat([self.act, self.act], dim=0), torch.cat([self.table, self.table], dim=0), self.widths)


class ResnetBlock2D(nn.Module):
    def __init__(self, cin, cout, temb_dim, groups=32, eps=1e-5):
        super().__init__()
        self.norm1 = nn.GroupNorm(groups, cin, eps=eps)
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1)
        self.time_emb_proj = nn.Linear(temb_dim, cout)
        self.norm2 = nn.GroupNorm(groups, cout, eps=eps)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
        self.conv_shortcut = nn.Conv2d(cin, cout, 1) if cin != cout else None

    def forward(self, x, temb_act):
        h = self.conv1(gn_act(x, self.norm1))
        h = self.conv2(gn_act(h, self.norm2, pre_bias=self.time_emb_proj(temb_act)))     # temb add folded into the norm kernel
        return (x if self.conv_shortcut is None else self.conv_shortcut(x)) + h

    def forward_pf(self, x, temb_act, x2=None):
        """x2: optional second PF tensor -- the block's input is the channel concatenation [x | x2] (a skip connection), which is
        never materialised: GroupNorm and the shortcut read both tensors in place."""
        cout = self.conv2.out_channels
        fuse = self.conv_shortcut is not None and pf.conv3x3_res_fusable(x, cout) and (x2 is None or x2.C % 64 == 0)
        if x2 is not None and not fuse:
            x, x2 = pf.PF(torch.cat([x.buf, x2.buf], dim=1), x.B, x.H, x.W, x.C + x2.C), None
        n1 = pf.groupnorm_pf2(x, x2, self.norm1.weight, self.norm1.bias, self.norm1.num_groups, self.norm1.eps, act=True)
        rowbias = temb_act.rows[id(self)] if isinstance(temb_act, TembRows) else _lin(temb_act, self.time_emb_proj).contiguous()
        h = pf.conv_pf(n1, _pw(self.conv1), self.conv1.bias, rowbias=rowbias, gn_only=True)       # read by norm2 and nothing else: no border zeroing when it wrote records
        h = pf.gn_pf(h, self.norm2)
        if self.conv_shortcut is None:
            return pf.conv_pf(h, _pw(self.conv2), self.conv2.bias, resid=x)                 # residual add in the GEMM epilogue
        if not fuse:
            sc = pf.conv_pf(x, _pw(self.conv_shortcut), self.conv_shortcut.bias, ksize=1)
            return pf.conv_pf(h, _pw(self.conv2), self.conv2.bias, resid=sc)
        c = pf.cached(self, "_gsw_res", (self.conv2.weight, self.conv2.bias, self.conv_shortcut.weight, self.conv_shortcut.bias),
                   lambda: (torch.cat([_pw(self.conv2), self.conv_shortcut.weight.detach()[:, :, 0, 0]], dim=1).contiguous(),      # [N, 9*C | C_shortcut]
                            (self.conv2.bias.detach() + self.conv_shortcut.bias.detach()).contiguous()))                           # summed biases
        return pf.conv3x3_res_pf(h, c[0], c[1], x1=x, x2=x2)                                # conv2 + conv_shortcut in one GEMM


def _padded_ctx(ctx: torch.Tensor):
    """Context tokens zero-padded to a multiple of 64 keys for the attention kernel (77 -> 128), computed once per context tensor:
    every cross-attention layer of every step receives the same object."""
    n = ctx.shape[1]
    if n % 64 == 0:
        return ctx, n
    cached = getattr(ctx, "_gsw_pad", None)              # (tensor version at padding time, padded copy)
    if cached is not None and cached[1].device == ctx.device and cached[1].dtype == ctx.dtype:
        if cached[0] == ctx._version:
            return cached[1], n
        # the context was edited in place: refresh the padded copy IN PLACE too, so that its address -- which a captured HIP graph of the
        # forward (graph.py) has baked in -- stays valid; in-place edits of ctx bump _version, the copy_ below bumps the pad's own
        cached[1][:, :n].copy_(ctx)
        ctx._gsw_pad = (ctx._version, cached[1])
        return cached[1], n
    pad = F.pad(ctx, (0, 0, 0, (-n) % 64)).contiguous()
    ctx._gsw_pad = (ctx._version, pad)
    return pad, n


def _padded_keys(ctx: torch.Tensor) -> int:
    """key count of _padded_ctx(ctx)"""
    return (ctx.shape[1] + 63) // 64 * 64


class Attention(nn.Module):
    def __init__(self, dim, ctx_dim, heads, head_dim):
        super().__init__()
        if head_dim is None:                     # SD 1.x: a fixed NUMBER of heads (8), head_dim = dim / heads (40 / 80 / 160)
            head_dim = dim // heads
        inner = heads * head_dim
        self.heads = heads
        self.to_q = nn.Linear(dim, inner, bias=False)
        self.to_k = nn.Linear(ctx_dim, inner, bias=False)
        self.to_v = nn.Linear(ctx_dim, inner, bias=False)
        self.to_out = nn.ModuleList([nn.Linear(inner, dim)])

    @property
    def head_dim(self) -> int:
        return self.to_q.out_features // self.heads

    def _no_qkv_bias(self) -> bool:
        return self.to_q.bias is None and self.to_k.bias is None and self.to_v.bias is None

    def _wcat(self, which: str) -> torch.Tensor:
        """The projection weights named by the letters of `which` ("qk" | "qkv") stacked row-wise, cached on the module (pf.cached, keyed by those weights)."""
        ws = tuple(getattr(self, "to_" + c).weight for c in which)
        return pf.cached(self, "_gsw_w" + which, ws, lambda: torch.cat([w.detach() for w in ws], dim=0).contiguous())

    def _folded(self, which: str, norm: nn.LayerNorm):
        """pf.fold_ln_weights of the projection(s) "q" | "qk" | "v" behind LayerNorm `norm`, cached on the module (keyed by the weights and the norm's parameters)."""
        ws = tuple(getattr(self, "to_" + c).weight for c in which)
        return pf.cached(self, "_gsw_ln_" + which, ws + (norm.weight, norm.bias),
                         lambda: pf.fold_ln_weights(ws[0].detach() if len(ws) == 1 else torch.cat([w.detach() for w in ws], dim=0), None, norm.weight, norm.bias))

    def context_kv(self, src: torch.Tensor):
        """Cross-attention keys / values^T of a (padded) context tensor: they depend on the context only, so they are computed once per
        (context tensor, layer) and reused by every step of a sampling / inversion loop.  The cache lives ON the context tensor (it dies with
        it) and is keyed by the tensor's and the weights' version counters, so in-place edits recompute it -- INTO the existing buffers: a
        captured HIP graph of the forward (graph.py) reads K / V^T at fixed addresses."""
        store = getattr(src, "_gsw_kv", None)
        if store is None:
            store = {}
            src._gsw_kv = store
        ver = (src._version, self.to_k.weight._version, self.to_v.weight._version, self.to_k.weight.data_ptr(), self.to_v.weight.data_ptr())
        ent = store.get(id(self))
        if ent is None or ent[0] != ver:
            ent = (ver, _lin(src, self.to_k, out=None if ent is None else ent[1]), _lin_t(src, self.to_v, out=None if ent is None else ent[2]))
            store[id(self)] = ent
        return ent[1], ent[2]

    def forward_ln(self, x, stat, norm: nn.LayerNorm, ctx=None, resid=None, project: bool = True):
        """attn(LayerNorm(x)) + resid with the LayerNorm folded into the projections that consume it (pf.gemm_ln): x is the RAW residual stream,
        stat its per-row (rstd, -rstd mean).  Self-attention: q | k and V^T; cross-attention: q (keys / values come from the context).
        project=False: the attention output BEFORE to_out (the caller hands it, to_out and the residual to the launch that consumes them: fused_sublayer)."""
        n = x.shape[1]
        inner = self.to_q.out_features
        if ctx is None:
            qk = pf.gemm_ln(x, stat, *self._folded("qk", norm))
            vt = pf.gemm_ln(x, stat, *self._folded("v", norm), mode="trans", tokens=n)
            o = pf.attention(qk[..., :inner], qk[..., inner:], vt, self.heads)
        else:
            src, valid = _padded_ctx(ctx)
            fq = self._folded("q", norm)
            k_ctx, vt_ctx = self.context_kv(src)
            o = pf.attention(pf.gemm_ln(x, stat, *fq), k_ctx, vt_ctx, self.heads, valid_keys=valid)
        if not project:
            return o
        return _lin(o, self.to_out[0], resid, rowstats=True)

    def fused_sublayer(self, x, stat, norm: nn.LayerNorm, ctx, eps_next: Optional[float] = None, pre=None):
        """x + attn(LayerNorm(x), ctx) as ONE launch (xattn.py / csrc/gswm_xattn.hip): x [B, S, 320] raw residual stream, stat its (rstd, -rstd mean), ctx
        [B or 2B, 77, D] (2B: classifier-free guidance on shared latents -> [2B, S, 320]).  eps_next: leave the statistics of the new rows for the next LayerNorm.
        pre = (o, to_out): the same launch also runs the output projection of the self-attention in front -- x is then that projection's RESIDUAL, o the
        attention output, and the stream x + to_out(o) the sublayer works on exists in registers only (stat is not needed)."""
        blob, v, idx = xattn.context_operands(self, norm, ctx, x.dtype)
        if pre is not None:
            return xattn.fused(x, None, blob, v, idx, ctx.shape[0], self.heads, eps_out=eps_next, pre_o=pre[0], pre_w=xattn.out_projection_operand(pre[1], x.dtype),
                               pre_eps=norm.eps)
        return xattn.fused(x, stat, blob, v, idx, ctx.shape[0], self.heads, eps_out=eps_next)

    def cross_dup(self, x, ctx, *, stat=None, norm: Optional[nn.LayerNorm] = None):
        """Classifier-free guidance with shared latents: x [B, S, C] holds the queries' input ONCE, ctx [2B, 77, D] = (uncond | text) contexts.  The
        query projection runs on B rows; the 77-key attention once per context half, both writing one [2B, S, C] tensor; -> attention output (before
        the output projection).  stat / norm: LayerNorm folded into the projection (x is the raw residual stream), else x is already normalised."""
        B = x.shape[0]
        src, valid = _padded_ctx(ctx)
        k_ctx, vt_ctx = self.context_kv(src)
        q = pf.gemm_ln(x, stat, *self._folded("q", norm)) if stat is not None else _lin(x, self.to_q)
        o = torch.empty((2 * B, x.shape[1], self.to_q.out_features), dtype=x.dtype, device=x.device)
        pf.attention(q, k_ctx[:B], vt_ctx[:B], self.heads, valid_keys=valid, out=o[:B])
        pf.attention(q, k_ctx[B:], vt_ctx[B:], self.heads, valid_keys=valid, out=o[B:])
        return o

    def ln_foldable(self, x, ctx=None) -> bool:
        n = x.shape[1]
        return (OWN_ATTENTION and FUSED_KERNELS and n % 8 == 0 and self._no_qkv_bias()
                and pf.attention_ok(x, self.heads, self.head_dim, n, n if ctx is None else _padded_keys(ctx)) and (ctx is None or CACHE_CONTEXT_KV)
                and _own_gemm_ok(x, self.to_q.in_features, self.to_q.out_features))

    def _qkv(self, x, src, cross: bool):
        """(q, k, V^T) as the attention kernel reads them, keys / values projected from `src` (the padded context, or x itself).  The value projection is
        computed transposed (V^T = W_v src^T, one GEMM either way) because the kernel consumes V^T tiles.  Tried in this order: cached context K / V^T
        (CACHE_CONTEXT_KV); q | k | V^T from one launch (FUSED_QKV); q | k from one GEMM + V^T (FUSED_QK); three projections."""
        n, inner = x.shape[1], self.to_q.out_features
        if cross and CACHE_CONTEXT_KV:
            k_ctx, vt_ctx = self.context_kv(src)
            return _lin(x, self.to_q), k_ctx, vt_ctx
        if (not cross and FUSED_QK and FUSED_QKV and self._no_qkv_bias() and (2 * inner) % 160 == 0 and n % 8 == 0
                and _own_gemm_ok(x, self.to_q.in_features, 3 * inner)):
            wqkv = self._wcat("qkv")
            if wqkv.dtype == x.dtype:
                qk, vt = pf.gemm_qkv(x.contiguous(), wqkv, 2 * inner)
                return qk[..., :inner], qk[..., inner:], vt
        vt = _lin_t(src, self.to_v)
        if not cross and FUSED_QK:
            wqk = self._wcat("qk")            # x is read once; the kernel takes q and k as column slices
            qk = pf.gemm(x.contiguous(), wqk, None) if _own_gemm_ok(x, wqk.shape[1], wqk.shape[0]) else F.linear(x, wqk)
            return qk[..., :inner], qk[..., inner:], vt
        return _lin(x, self.to_q), _lin(src, self.to_k), vt

    def forward(self, x, ctx=None, resid=None):
        """resid: added to the output projection (in its GEMM epilogue on the own path): `x + attn(norm(x))` of the transformer block"""
        b, n, _ = x.shape
        if OWN_ATTENTION and FUSED_KERNELS:
            src, valid = (x, n) if ctx is None else _padded_ctx(ctx)
            if pf.attention_ok(x, self.heads, self.head_dim, n, src.shape[1]):
                # hand-written flash-attention kernel (self- and cross-attention).  Padded context rows are zero and masked by `valid`.
                q, k, vt = self._qkv(x, src, ctx is not None)
                return _lin(pf.attention(q, k, vt, self.heads, valid_keys=valid), self.to_out[0], resid)
            if pf.half_gpu(x):
                _note_fallback(f"attention head_dim={self.head_dim} Sq={n} Sk={src.shape[1]}: torch SDPA")
        ctx = x if ctx is None else ctx
        q = _lin(x, self.to_q).view(b, n, self.heads, -1).transpose(1, 2)
        k = _lin(ctx, self.to_k).view(b, ctx.shape[1], self.heads, -1).transpose(1, 2)
        v = _lin(ctx, self.to_v).view(b, ctx.shape[1], self.heads, -1).transpose(1, 2)
        o = F.scaled_dot_product_attention(q, k, v)
        return _lin(o.transpose(1, 2).reshape(b, n, -1), self.to_out[0], resid)


class GEGLU(nn.Module):
    def __init__(self, dim, inner):
        super().__init__()
        self.proj = nn.Linear(dim, inner * 2)

    def forward(self, x):
        inner = self.proj.out_features // 2
        if _own_gemm_ok(x, self.proj.in_features, self.proj.out_features) and inner % 80 == 0:
            _wb(self.proj, x)                 # value * gelu(gate) in the GEMM epilogue: no [M, 2I] intermediate
            c = pf.cached(self, "_gsw_geglu", (self.proj.weight, self.proj.bias), lambda: pf.pack_geglu_weight(self.proj.weight.detach(), self.proj.bias.detach()))
            return pf.gemm(x.contiguous(), c[0], c[1], mode="geglu")
        y = self.proj(x)
        if FUSED_KERNELS and y.is_cuda and y.is_contiguous() and (y.shape[-1] // 2) % 8 == 0:
            return codec.geglu(y)
        h, gate = y.chunk(2, dim=-1)
        return h * F.gelu(gate)


class FeedForward(nn.Module):
    def __init__(self, dim, mult=4):
        super().__init__()
        self.net = nn.ModuleList([GEGLU(dim, dim * mult), nn.Identity(), nn.Linear(dim * mult, dim)])

    def forward(self, x, resid=None, rowstats: bool = False):
        return _lin(self.net[0](x), self.net[2], resid, rowstats=rowstats)

    def _folded(self, norm: nn.LayerNorm):
        """pf.fold_ln_weights of the GEGLU projection behind LayerNorm `norm`, cached on the module (keyed by the projection's and the norm's parameters)."""
        proj = self.net[0].proj
        return pf.cached(self, "_gsw_ln_ff1", (proj.weight, proj.bias, norm.weight, norm.bias),
                         lambda: pf.fold_ln_weights(proj.weight.detach(), proj.bias, norm.weight, norm.bias, geglu=True))

    def forward_ln(self, x, stat, norm: nn.LayerNorm, resid=None):
        """ff(LayerNorm(x)) + resid with the LayerNorm folded into the GEGLU projection (pf.gemm_ln)"""
        return _lin(pf.gemm_ln(x, stat, *self._folded(norm), mode="geglu"), self.net[2], resid, rowstats=True)


def _fused_block_ok(like: torch.Tensor, channels: int) -> bool:
    """Tokens [B, S, channels] with the dtype and device of `like` (the tokens themselves, or the latent they will be made from) run the fused transformer
    block of BasicTransformerBlock.forward; the token tensor must be contiguous as well (BasicTransformerBlock.fused_ok)."""
    return FUSED_KERNELS and pf.half_gpu(like) and channels % 8 == 0 and channels <= 1536


def _cached_kv_on() -> bool:
    """the switches behind cross-attention on the own kernel with per-context cached K / V^T"""
    return OWN_ATTENTION and FUSED_KERNELS and CACHE_CONTEXT_KV


class BasicTransformerBlock(nn.Module):
    def __init__(self, dim, ctx_dim, heads, head_dim):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn1 = Attention(dim, dim, heads, head_dim)
        self.norm2 = nn.LayerNorm(dim)
        self.attn2 = Attention(dim, ctx_dim, heads, head_dim)
        self.norm3 = nn.LayerNorm(dim)
        self.ff = FeedForward(dim)

    @staticmethod
    def fused_ok(x) -> bool:
        """this token tensor runs the fused block (else the plain torch modules)"""
        return _fused_block_ok(x, x.shape[-1]) and x.is_contiguous()

    def dup_ok(self, x, ctx) -> bool:
        """forward(x, ctx, dup=True) is available: the fused path with the own attention kernel and cached context K / V, ctx holding two contexts per row of x"""
        a = self.attn2
        return (self.fused_ok(x) and _cached_kv_on() and ctx.shape[0] == 2 * x.shape[0]
                and pf.attention_ok(x, a.heads, a.head_dim, x.shape[1], _padded_keys(ctx)))

    def _cross_sublayer(self, x, ctx, dup: bool, one_launch: bool):
        """x + attn2(norm2(x), ctx) on the hand-written path; dup: x holds B rows, ctx 2B -> 2B rows"""
        st = pf.ln_stat(x, self.norm2.eps) if (one_launch or self.attn2.ln_foldable(x, ctx[: x.shape[0]] if dup else ctx)) else None
        if st is not None and one_launch:
            return self.attn2.fused_sublayer(x, st, self.norm2, ctx, eps_next=self.norm3.eps)
        if dup:
            if st is not None:
                o = self.attn2.cross_dup(x, ctx, stat=st, norm=self.norm2)
            else:
                _, n = codec.add_layernorm(x, None, self.norm2.weight, self.norm2.bias, self.norm2.eps)
                o = self.attn2.cross_dup(n, ctx)
            return _lin(o, self.attn2.to_out[0], torch.cat([x, x], dim=0), rowstats=True)
        if st is not None:
            return self.attn2.forward_ln(x, st, self.norm2, ctx, resid=x)
        _, n = codec.add_layernorm(x, None, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        return self.attn2(n, ctx, resid=x)

    def forward(self, x, ctx, dup: bool = False, ff_split: bool = False):
        """dup (classifier-free guidance, see UNet2DCondition.forward): x [B, S, C], ctx [2B, ...] -> [2B, S, C]; self-attention and the cross-attention
        queries are computed once on the B rows the two halves share.
        ff_split (fused path only; Transformer2DModel's last block): stop in front of ff.net[2] and return (h, x) -- the GEGLU hidden tensor and the residual
        stream -- for a caller that folds net[2] into the linear map that follows (the block's result would be x + ff.net[2](h))."""
        if dup and not self.dup_ok(x, ctx):
            x, dup = torch.cat([x, x], dim=0), False
        if not self.fused_ok(x):
            if ff_split:
                raise RuntimeError("BasicTransformerBlock: ff_split is a form of the fused path")
            x = x + self.attn1(self.norm1(x))
            x = x + self.attn2(self.norm2(x), ctx)
            return x + self.ff(self.norm3(x))
        # the residual adds ride in the output projections' GEMM epilogues.  Each LayerNorm is FOLDED into the projections that consume it when the
        # launch that produced x left row records on it (large batches: pf.ln_stat) -- the normalised tensor is then never written; otherwise it is
        # one read + one write (gsw_add_layernorm)
        one_launch = xattn.usable(x, self.attn2, ctx)      # the 320-channel level: norm2 + query projection + 77-key attention + output projection + residual in one kernel
        st = pf.ln_stat(x, self.norm1.eps) if self.attn1.ln_foldable(x) else None
        if st is not None and one_launch and xattn.pre_usable(self.attn1.to_out[0]):
            # ... and the self-attention's output projection + bias + residual + norm2's statistics as that kernel's prologue: the stream between the two
            # attention sublayers is never stored (dup: the launch writes 2B rows from B)
            o1 = self.attn1.forward_ln(x, st, self.norm1, project=False)
            x = self.attn2.fused_sublayer(x, None, self.norm2, ctx, eps_next=self.norm3.eps, pre=(o1, self.attn1.to_out[0]))
        else:
            if st is not None:
                x = self.attn1.forward_ln(x, st, self.norm1, resid=x)
            else:
                _, n = codec.add_layernorm(x, None, self.norm1.weight, self.norm1.bias, self.norm1.eps)
                x = self.attn1(n, resid=x)
            x = self._cross_sublayer(x, ctx, dup, one_launch)
        inner4 = self.ff.net[2].in_features
        st = pf.ln_stat(x, self.norm3.eps) if (inner4 % 80 == 0 and _own_gemm_ok(x, x.shape[-1], 2 * inner4)) else None
        if st is not None:
            if ff_split:
                return pf.gemm_ln(x, st, *self.ff._folded(self.norm3), mode="geglu"), x
            return self.ff.forward_ln(x, st, self.norm3, resid=x)
        _, n = codec.add_layernorm(x, None, self.norm3.weight, self.norm3.bias, self.norm3.eps)
        if ff_split:
            return self.ff.net[0](n), x
        return self.ff(n, resid=x)


def fold_ff_out(w2: torch.Tensor, b2: torch.Tensor, wp: torch.Tensor, bp: torch.Tensor):
    """Two linear maps with nothing between them as one: proj_out(x + ff.net[2](h)) = [h | x] W_cat^T + b' with W_cat = [Wp W2 | Wp] ([C, 5C]) and
    b' = Wp b2 + bp.  The products are formed in fp32 (fp64 parameters: fp64) and rounded ONCE to the parameters' dtype."""
    acc = torch.float64 if wp.dtype == torch.float64 else torch.float32
    wpf, w2f = wp.detach().to(acc), w2.detach().to(acc)
    w_cat = torch.cat([wpf @ w2f, wpf], dim=1).to(wp.dtype).contiguous()
    b = (wpf @ b2.detach().to(acc) + bp.detach().to(acc)).to(wp.dtype).contiguous()
    return w_cat, b


class Transformer2DModel(nn.Module):
    def __init__(self, ch, ctx_dim, heads, head_dim, layers=1, groups=32):
        super().__init__()
        self.norm = nn.GroupNorm(groups, ch, eps=1e-6)
        self.proj_in = nn.Linear(ch, ch)        # use_linear_projection=True (SD 2.x)
        self.transformer_blocks = nn.ModuleList([BasicTransformerBlock(ch, ctx_dim, heads, head_dim) for _ in range(layers)])
        self.proj_out = nn.Linear(ch, ch)

    def forward(self, x, ctx):
        b, c, h, w = x.shape
        y = gn_act(x, self.norm, act=False).permute(0, 2, 3, 1).reshape(b, h * w, c)
        y = self.proj_in(y)
        for blk in self.transformer_blocks:
            y = blk(y, ctx)
        y = self.proj_out(y).reshape(b, h, w, c).permute(0, 3, 1, 2)
        return x + y

    def _ff_out_folded(self):
        """fold_ff_out of the last block's ff.net[2] and proj_out, cached on the module (keyed by the four parameters)"""
        l2, po = self.transformer_blocks[-1].ff.net[2], self.proj_out
        return pf.cached(self, "_gsw_ff_out", (l2.weight, l2.bias, po.weight, po.bias), lambda: fold_ff_out(l2.weight, l2.bias, po.weight, po.bias))

    def _ff_out_fold_ok(self, y, dup: bool) -> bool:
        """The last block's ff.net[2] and proj_out run as one two-segment launch (FOLD_FF_OUT): tokens y [B, S, C] on the fused block path, both linears on
        the matmul engine -- the small-batch kernel (at most pf.SMALL_GEMM_MAX_ROWS rows) keeps the two launches."""
        C = self.proj_out.in_features
        if not (FOLD_FF_OUT and len(self.transformer_blocks) > 0 and C % 64 == 0):
            return False
        l2 = self.transformer_blocks[-1].ff.net[2]
        rows = y.shape[0] * y.shape[1] * (2 if dup else 1)
        return (BasicTransformerBlock.fused_ok(y) and l2.bias is not None and self.proj_out.bias is not None and l2.out_features == C and l2.in_features % 64 == 0
                and self.proj_out.out_features == C and rows > pf.SMALL_GEMM_MAX_ROWS and _own_gemm_ok(y, l2.in_features, C) and _own_gemm_ok(y, C, C))

    def forward_pf(self, x, ctx, dup: bool = False):
        """dup: x holds B images, ctx 2B contexts -> a PF tensor of 2B images (see UNet2DCondition.forward)"""
        if xattn.gn_proj_usable(x, self.norm, self.proj_in):
            # the 320-channel level at large batch: GroupNorm + proj_in in one launch, the rows normalised on their way into the matrix pipe (never stored)
            y = xattn.gn_proj(x, self.norm, self.proj_in, eps_next=self.transformer_blocks[0].norm1.eps)
        else:
            y = _lin(pf.gn_pf(x, self.norm, act=False, tokens=True), self.proj_in, rowstats=True)      # GroupNorm writes dense tokens directly
        last = len(self.transformer_blocks) - 1
        fold = self._ff_out_fold_ok(y, dup)
        for i, blk in enumerate(self.transformer_blocks):
            y = blk(y, ctx, dup=dup and i == 0, ff_split=fold and i == last)
        if dup:
            x = pf.dup_pf(x)
        if fold:
            # proj_out(y + ff.net[2](h)) + residual as ONE launch over the two A operands (h, y): the last block's output is never written.  net[2]'s row
            # records are not requested either -- nothing normalises the stream behind the last block
            h, y = y
            w, b = self._ff_out_folded()
            pf.gemm2(h.contiguous(), y.contiguous(), w, b, resid=x.rows, mode="tok2pf", tokens=x.H * x.W, width=x.W, out=x.rows, stats_for=x)
        elif _own_gemm_ok(y, self.proj_out.in_features, self.proj_out.out_features):
            w, b = _wb(self.proj_out, y)        # proj_out + residual written straight into the PF tensor's interior rows (x has no other reader)
            pf.gemm(y.contiguous(), w, b, resid=x.rows, mode="tok2pf", tokens=x.H * x.W, width=x.W, out=x.rows, stats_for=x)
        else:
            x.interior.add_(_lin(y, self.proj_out).view(x.B, x.H, x.W, x.C))
            x.stats = None
        return x


class Downsample2D(nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.conv = nn.Conv2d(ch, ch, 3, stride=2, padding=1)

    def forward(self, x):
        return self.conv(x)

    def forward_pf(self, x):
        return pf.conv_pf(x, _pw(self.conv), self.conv.bias, stride=2)


class Upsample2D(nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.conv = nn.Conv2d(ch, ch, 3, padding=1)

    def forward(self, x):
        return self.conv(F.interpolate(x, scale_factor=2.0, mode="nearest"))

    def forward_pf(self, x):
        if UPSAMPLE_SUBPIXEL and pf.conv_up2x_fusable(x, self.conv.out_channels):
            w4 = pf.cached(self, "_gsw_up4", (self.conv.weight,), lambda: pf.pack_upsample_weight(self.conv.weight))
            return pf.conv_up2x_pf(x, w4, self.conv.bias)            # 2.25x fewer FLOPs, no upsampled intermediate
        up = pf.PF.zeros(x.B, 2 * x.H, 2 * x.W, x.C, x.buf.dtype, x.buf.device)
        xi, g = x.interior, up.grid
        for dy in (0, 1):
            for dx in (0, 1):
                g[:, 1 + dy:1 + dy + 2 * x.H:2, 1 + dx:1 + dx + 2 * x.W:2, :].copy_(xi)
        return pf.conv_pf(up, _pw(self.conv), self.conv.bias)


class DownBlock(nn.Module):
    def __init__(self, cin, cout, temb, ctx_dim, heads, head_dim, layers, attn, down):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(cin if i == 0 else cout, cout, temb) for i in range(layers)])
        self.attentions = nn.ModuleList([Transformer2DModel(cout, ctx_dim, heads, head_dim) for _ in range(layers)]) if attn else None
        self.downsamplers = nn.ModuleList([Downsample2D(cout)]) if down else None

    def forward(self, x, temb, ctx, skips):
        for i, r in enumerate(self.resnets):
            x = r(x, temb)
            if self.attentions is not None:
                x = self.attentions[i](x, ctx)
            skips.append(x)
        if self.downsamplers is not None:
            x = self.downsamplers[0](x)
            skips.append(x)
        return x

    def forward_pf(self, x, temb, ctx, skips, dup_temb=None):
        """dup_temb (first down block under classifier-free guidance with shared latents): x holds B images, ctx 2B contexts; the first resnet and the
        first transformer up to its cross-attention run on B images, everything after on 2B with the doubled time-embedding rows `dup_temb`"""
        for i, r in enumerate(self.resnets):
            x = r.forward_pf(x, temb)
            if self.attentions is not None:
                x = self.attentions[i].forward_pf(x, ctx, dup=dup_temb is not None and i == 0)
                if dup_temb is not None and i == 0:
                    temb = dup_temb
            skips.append(x)
        if self.downsamplers is not None:
            x = self.downsamplers[0].forward_pf(x)
            skips.append(x)
        return x


class UpBlock(nn.Module):
    def __init__(self, cin, cout, cprev, temb, ctx_dim, heads, head_dim, layers, attn, up):
        super().__init__()
        rs = []
        for i in range(layers):
            skip = cin if i == layers - 1 else cout
            rin = cprev if i == 0 else cout
            rs.append(ResnetBlock2D(rin + skip, cout, temb))
        self.resnets = nn.ModuleList(rs)
        self.attentions = nn.ModuleList([Transformer2DModel(cout, ctx_dim, heads, head_dim) for _ in range(layers)]) if attn else None
        self.upsamplers = nn.ModuleList([Upsample2D(cout)]) if up else None

    def forward(self, x, temb, ctx, skips):
        for i, r in enumerate(self.resnets):
            x = r(torch.cat([x, skips.pop()], dim=1), temb)
            if self.attentions is not None:
                x = self.attentions[i](x, ctx)
        if self.upsamplers is not None:
            x = self.upsamplers[0](x)
        return x

    def forward_pf(self, x, temb, ctx, skips):
        for i, r in enumerate(self.resnets):
            x = r.forward_pf(x, temb, x2=skips.pop())
            if self.attentions is not None:
                x = self.attentions[i].forward_pf(x, ctx)
        if self.upsamplers is not None:
            x = self.upsamplers[0].forward_pf(x)
        return x


class MidBlock(nn.Module):
    def __init__(self, ch, temb, ctx_dim, heads, head_dim):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(ch, ch, temb), ResnetBlock2D(ch, ch, temb)])
        self.attentions = nn.ModuleList([Transformer2DModel(ch, ctx_dim, heads, head_dim)])

    def forward(self, x, temb, ctx):
        return self.resnets[1](self.attentions[0](self.resnets[0](x, temb), ctx), temb)

    def forward_pf(self, x, temb, ctx):
        return self.resnets[1].forward_pf(self.attentions[0].forward_pf(self.resnets[0].forward_pf(x, temb), ctx), temb)


TEMB_TABLE = True     # integer timesteps: the whole time-embedding chain (sinusoid -> linear -> SiLU -> linear -> SiLU -> every resnet's time_emb_proj) is a
                      # function of t alone -- tabulated once over the training timesteps, a forward gathers its rows (one launch instead of ~20, and the
                      # 50 MB of projection weights are not streamed per forward)
NUM_TRAIN_TIMESTEPS = 1000   # default length of the table; a model built from a checkpoint carries its scheduler's value as `model.num_train_timesteps`
                             # (extract.Models sets it from scheduler/scheduler_config.json), and ddim.DDIMSchedule refuses timesteps outside the range on the host

CONV_OUT_DIRECT_MAX_PIXELS = 65536      # conv_out (320 -> 4) as the one-wave-per-16-pixels kernel writing NCHW directly (gsw_conv3x3_pf_nchw); above that the
                                        # LDS-tiled 64-column kernel moves fewer bytes through L2

CFG_SHARED_PREFIX = os.environ.get("GSW_CFG_SHARED_PREFIX", "1") != "0"      # classifier-free guidance: the part of a forward that does not see the context runs once for both halves of the batch


def _edge_conv_weights(self):
    """conv_in (4 -> 320) and conv_out (320 -> 4) for the PF GEMM: the 4-channel side is zero-padded to one 64-wide tile."""
    w_in, w_out = self.conv_in.weight, self.conv_out.weight

    def build():
        wi = torch.zeros((w_in.shape[0], 64, 3, 3), dtype=w_in.dtype, device=w_in.device)
        wi[:, : w_in.shape[1]] = w_in.detach()
        wo = torch.zeros((64, w_out.shape[1], 3, 3), dtype=w_out.dtype, device=w_out.device)
        wo[: w_out.shape[0]] = w_out.detach()
        bo = torch.zeros(64, dtype=w_out.dtype, device=w_out.device)
        bo[: w_out.shape[0]] = self.conv_out.bias.detach()
        return pf.pack_conv_weight(wi), pf.pack_conv_weight(wo), bo

    return pf.cached(self, "_gsw_edge", (w_in, w_out, self.conv_out.bias), build)


def _resnets(self):
    """every ResnetBlock2D of the model, in module order (= the column order of the time-embedding rows)"""
    resnets = getattr(self, "_gsw_resnets", None)
    if resnets is None:
        resnets = self._gsw_resnets = [m for m in self.modules() if isinstance(m, ResnetBlock2D)]
    return resnets


def _temb_widths(resnets):
    return [(id(r), r.time_emb_proj.out_features) for r in resnets]


def _temb_rows(self, temb: torch.Tensor):
    """Every resnet's time_emb_proj(temb) from one GEMM over the row-concatenated weights -> TembRows (or temb itself off the engine)."""
    resnets = _resnets(self)
    widths = _temb_widths(resnets)
    if not resnets or not _own_gemm_ok(temb, temb.shape[-1], sum(n for _, n in widths)) or any(n % 8 for _, n in widths):
        return temb
    params = tuple(p for r in resnets for p in (r.time_emb_proj.weight, r.time_emb_proj.bias))
    wcat, bcat = pf.cached(self, "_gsw_temb_cat", params, lambda: (torch.cat([r.time_emb_proj.weight.detach() for r in resnets], dim=0).contiguous(),
                                                                     torch.cat([r.time_emb_proj.bias.detach() for r in resnets], dim=0).contiguous()))
    if wcat.dtype != temb.dtype:
        return temb
    return TembRows(temb, pf.gemm(temb.contiguous(), wcat, bcat), widths)


def _temb_rows_from_table(self, t: torch.Tensor, x: torch.Tensor):
    """TembRows gathered from the per-model table [num_train_timesteps, sum of the resnets' channels], or None when t is not an integer tensor / the
    projections do not run on the engine.  The table is as long as the model's `num_train_timesteps` (the scheduler config's; 1000 by default).  The
    schedules of ddim.py validate their timesteps against that range on the host; a device tensor outside it would be clamped by gsw_gather_rows."""
    if t.dtype not in (torch.int64, torch.int32) or not t.is_cuda or t.numel() not in (1, x.shape[0]):
        return None
    resnets = _resnets(self)
    if not resnets or any(r.time_emb_proj.out_features % 8 for r in resnets):
        return None
    te = self.time_embedding
    if te.linear_1.weight.dtype != x.dtype or te.linear_1.weight.device != x.device:
        return None
    params = (te.linear_1.weight, te.linear_1.bias, te.linear_2.weight, te.linear_2.bias) + tuple(p for r in resnets for p in (r.time_emb_proj.weight, r.time_emb_proj.bias))

    def build():
        with torch.no_grad():
            tt = torch.arange(int(getattr(self, "num_train_timesteps", NUM_TRAIN_TIMESTEPS)), device=x.device)
            temb = F.silu(te(timestep_embedding(tt, self.c0).to(x.dtype)))
            rows = _temb_rows(self, temb)
            if not isinstance(rows, TembRows):
                return None
            return rows.table.contiguous()

    table = pf.cached(self, "_gsw_temb_table", params, build)
    if table is not None and table.shape[0] != int(getattr(self, "num_train_timesteps", NUM_TRAIN_TIMESTEPS)):      # the scheduler length changed after the table was built
        self._gsw_temb_table = None
        table = pf.cached(self, "_gsw_temb_table", params, build)
        graph.weights_changed()      # a captured forward gathers from the OLD table's address: every graph entry must re-capture
    if table is None:
        return None
    B, n_tot = x.shape[0], table.shape[1]
    idx = t if t.dtype == torch.int64 else t.to(torch.int64)
    out = torch.empty((B, n_tot), dtype=table.dtype, device=table.device)
    with torch.cuda.device(x.device):
        N.check(N.lib().gsw_gather_rows(table.data_ptr(), n_tot * table.element_size(), table.shape[0], idx.data_ptr(), 0 if idx.numel() == 1 else 1,
                                        out.data_ptr(), n_tot * table.element_size(), B, n_tot * table.element_size(), codec._stream_ptr()))
    return TembRows(None, out, _temb_widths(resnets))


class UNet2DCondition(nn.Module):
    """SD 2.1-base shape by default (865.9 M parameters); `UNet2DCondition.sd15()` gives the SD 1.5 shape of BASELINE config 5."""

    @classmethod
    def sd15(cls) -> "UNet2DCondition":
        """runwayml/stable-diffusion-v1-5 `unet/config.json`: 8 heads everywhere (head_dim 40/80/160/160), cross_attention_dim 768.
        Its proj_in / proj_out are 1x1 convolutions, numerically the linear layers used here (load_diffusers_state_dict squeezes
        the [C, C, 1, 1] weights)."""
        return cls(cross_attention_dim=768, num_heads=(8, 8, 8, 8), head_dim=None)

    def __init__(self, in_channels=4, out_channels=4, block_out_channels: Sequence[int] = (320, 640, 1280, 1280), layers_per_block=2,
                 cross_attention_dim=1024, num_heads: Sequence[int] = (5, 10, 20, 20), head_dim=64,
                 attn_blocks: Sequence[bool] = (True, True, True, False)):
        super().__init__()
        c0 = block_out_channels[0]
        temb = c0 * 4
        self.c0 = c0
        self.conv_in = nn.Conv2d(in_channels, c0, 3, padding=1)
        self.time_embedding = TimestepEmbedding(c0, temb)
        self.down_blocks = nn.ModuleList()
        ch = c0
        n = len(block_out_channels)
        for i, co in enumerate(block_out_channels):
            self.down_blocks.append(DownBlock(ch, co, temb, cross_attention_dim, num_heads[i], co // num_heads[i] if head_dim is None else head_dim,
                                              layers_per_block, attn_blocks[i], i < n - 1))
            ch = co
        self.mid_block = MidBlock(ch, temb, cross_attention_dim, num_heads[-1], head_dim)
        self.up_blocks = nn.ModuleList()
        rev = list(reversed(block_out_channels))
        rheads = list(reversed(num_heads))
        rattn = list(reversed(attn_blocks))
        cprev = ch
        for i, co in enumerate(rev):
            cin = rev[min(i + 1, n - 1)]
            self.up_blocks.append(UpBlock(cin, co, cprev, temb, cross_attention_dim, rheads[i], head_dim, layers_per_block + 1, rattn[i], i < n - 1))
            cprev = co
        self.conv_norm_out = nn.GroupNorm(32, c0, eps=1e-5)
        self.conv_out = nn.Conv2d(c0, out_channels, 3, padding=1)

    supports_cfg_dup = True

    def forward(self, x: torch.Tensor, t: torch.Tensor, ctx: torch.Tensor, cfg_dup: bool = False) -> torch.Tensor:
        """x [B,4,h,w], t [B] (or scalar tensor) timesteps, ctx [B,77,1024] -> model output [B,4,h,w].
        cfg_dup (classifier-free guidance, the reference's `torch.cat([latents] * 2)` of modified_stable_diffusion_gs.pyc): ctx holds 2B contexts
        (uncond | text) for the SAME B latents -> output [2B,4,h,w].  Until the first cross-attention the two halves of the batch are the same
        numbers -- conv_in, the first resnet, the first transformer's GroupNorm / proj_in / self-attention / query projection -- so they are computed
        once on B rows (CFG_SHARED_PREFIX; per-row results are what the doubled batch would compute)."""
        if cfg_dup:
            if ctx.shape[0] != 2 * x.shape[0] or t.numel() not in (1, x.shape[0]):
                raise ValueError("cfg_dup: ctx must hold 2B contexts for the B latents, t one timestep or B")
            if not (CFG_SHARED_PREFIX and self._pf_ok(x) and self._cfg_dup_ok(x, ctx)):
                return self.forward(torch.cat([x, x], dim=0), t if t.numel() == 1 else torch.cat([t, t]), ctx)
        if self._pf_ok(x):
            rows = _temb_rows_from_table(self, t, x) if TEMB_TABLE else None
            if rows is not None:
                return self._forward_pf(x, rows, ctx, cfg_dup)
        if t.dim() == 0:
            t = t.expand(x.shape[0])
        temb = self.time_embedding(timestep_embedding(t, self.c0).to(x.dtype))
        temb = F.silu(temb)                      # every resnet applies SiLU to the same embedding: do it once
        if self._pf_ok(x):
            return self._forward_pf(x, _temb_rows(self, temb), ctx, cfg_dup)
        if USE_PF and FUSED_KERNELS and pf.half_gpu(x):
            _note_fallback(f"UNet forward on {tuple(x.shape)} {x.dtype}: off the padded-flat path (fp16 / bf16, conv channels % 64, lattice % {1 << (len(self.down_blocks) - 1)}): plain torch modules")
        h = self.conv_in(x)
        skips = [h]
        for blk in self.down_blocks:
            h = blk(h, temb, ctx, skips)
        h = self.mid_block(h, temb, ctx)
        for blk in self.up_blocks:
            h = blk(h, temb, ctx, skips)
        # the scheduler-step / vote kernels index the lattice in C order: hand back plain NCHW even when the convolutions
        # run channels-last
        return self.conv_out(gn_act(h, self.conv_norm_out)).contiguous(memory_format=torch.contiguous_format)

    def _pf_ok(self, x: torch.Tensor) -> bool:
        if not (USE_PF and FUSED_KERNELS and pf.half_gpu(x)):
            return False
        ok = getattr(self, "_pf_shapes_ok", None)
        if ok is None:
            ok = all(m.in_channels % 64 == 0 and m.out_channels % 64 == 0 for n, m in self.named_modules()
                     if isinstance(m, nn.Conv2d) and n not in ("conv_in", "conv_out"))
            self._pf_shapes_ok = ok
        n_down = len(self.down_blocks) - 1
        return ok and x.shape[-1] % (1 << n_down) == 0 and x.shape[-2] % (1 << n_down) == 0

    def _cfg_dup_ok(self, x: torch.Tensor, ctx: torch.Tensor) -> bool:
        """forward(cfg_dup=True) may share the prefix.  Asked from the latent, before any token tensor exists: the shape / dtype / device terms and switches of
        BasicTransformerBlock.dup_ok for the first transformer block (not its contiguity or row-count terms), plus OWN_GEMM and the query projection on the engine."""
        b0 = self.down_blocks[0]
        if b0.attentions is None or not isinstance(b0.attentions[0].transformer_blocks[0], BasicTransformerBlock):
            return False
        a = b0.attentions[0].transformer_blocks[0].attn2
        return (_fused_block_ok(x, b0.attentions[0].proj_in.out_features) and _cached_kv_on() and OWN_GEMM and a.head_dim in pf.ATTN_HEAD_DIMS
                and _own_gemm_ok(x, a.to_q.in_features, a.to_q.out_features))

    def _forward_pf(self, x: torch.Tensor, temb, ctx: torch.Tensor, cfg_dup: bool = False) -> torch.Tensor:
        w_in, w_out, b_out = _edge_conv_weights(self)
        B, cin, H, W = x.shape
        xin = pf.PF.empty(B, H, W, 64, x.dtype, x.device)
        xc = x.contiguous()
        with torch.cuda.device(x.device):
            N.check(N.lib().gsw_nchw_to_pf(xc.data_ptr(), xin.rows.data_ptr(), B, cin, H, W, 64, codec._dt(x.dtype), codec._stream_ptr()))
        h = pf.conv_pf(xin, w_in, self.conv_in.bias)
        skips = [h]
        if cfg_dup:
            temb2 = temb.doubled() if isinstance(temb, TembRows) else torch.cat([temb, temb], dim=0)      # the time-embedding rows of the doubled batch
            h = self.down_blocks[0].forward_pf(h, temb, ctx, skips, dup_temb=temb2)
            skips[0] = pf.dup_pf(skips[0])              # the conv_in skip is consumed by the last up-block resnet, on 2B images
            temb, B = temb2, 2 * B
            rest = self.down_blocks[1:]
        else:
            rest = self.down_blocks
        for blk in rest:
            h = blk.forward_pf(h, temb, ctx, skips)
        h = self.mid_block.forward_pf(h, temb, ctx)
        for blk in self.up_blocks:
            h = blk.forward_pf(h, temb, ctx, skips)
        hn = pf.gn_pf(h, self.conv_norm_out, act=True)
        nout = self.conv_out.out_channels
        if B * H * W <= CONV_OUT_DIRECT_MAX_PIXELS and nout <= 16 and hn.C % 32 == 0 and self.conv_out.bias is not None:
            wo = pf.cached(self.conv_out, "_gsw_packed_direct", (self.conv_out.weight,), lambda: pf.pack_conv_weight(self.conv_out.weight.detach()))
            y = torch.empty((B, nout, H, W), dtype=x.dtype, device=x.device)
            with torch.cuda.device(x.device):
                N.check(N.lib().gsw_conv3x3_pf_nchw(hn.rows.data_ptr(), wo.data_ptr(), self.conv_out.bias.data_ptr(), y.data_ptr(), B, H, W, hn.C, nout,
                                                    codec._dt(x.dtype), codec._stream_ptr()))
            return y
        y = pf.conv_pf(hn, w_out, b_out)
        return y.interior[..., :nout].permute(0, 3, 1, 2).contiguous()

    def prepare_context(self, ctx: torch.Tensor) -> None:
        """Bring the per-context caches (padded copy, every cross-attention layer's K / V^T) up to date for `ctx` without running a forward --
        in place when they exist (graph.py calls this after overwriting a captured graph's static context buffer)."""
        if not (_cached_kv_on() and ctx.is_cuda):
            return
        src, _ = _padded_ctx(ctx)
        for blk in self.modules():
            if isinstance(blk, BasicTransformerBlock):
                a = blk.attn2
                if pf.attention_ok(ctx, a.heads, a.head_dim, 1, src.shape[1]):
                    a.context_kv(src)
                if xattn.layer_usable(a, ctx, ctx.dtype):
                    xattn.context_operands(a, blk.norm2, ctx, ctx.dtype)      # the one-launch cross-attention's per-context fragment streams
                    if xattn.pre_usable(blk.attn1.to_out[0]):
                        xattn.out_projection_operand(blk.attn1.to_out[0], ctx.dtype)      # ... and the prologue's (the self-attention's output projection; per layer, not per context)


def synthetic_init_(model: nn.Module, seed: int = 0, out_scale: float = 1.0) -> nn.Module:
    """Deterministic synthetic weights (no checkpoint is reachable from here): fan-in scaled normal for matrices/convs,
    ones/zeros for norms.  Residual-branch output layers are down-scaled so activations stay O(1) through ~60 residual
    adds, which keeps fp16 in range like a trained network does."""
    g = torch.Generator().manual_seed(seed)
    n_res = 0
    for name, p in model.named_parameters():
        if p.dim() >= 2:
            fan_in = p[0].numel()
            std = (1.0 / fan_in) ** 0.5
            if name.endswith(("conv2.weight", "to_out.0.weight", "net.2.weight", "proj_out.weight")):
                std *= 0.3
                n_res += 1
            if name == "conv_out.weight":
                std *= out_scale
            with torch.no_grad():
                p.copy_(torch.randn(p.shape, generator=g) * std)
        else:
            with torch.no_grad():
                p.fill_(1.0 if name.endswith("weight") and "norm" in name else 0.0)
    return model


def load_diffusers_state_dict(model: nn.Module, weight_dir: str) -> nn.Module:
    """Load the UNet weights of a diffusers-layout directory (`<weight_dir>/unet/diffusion_pytorch_model.*`: safetensors, sharded safetensors or .bin,
    checkpoint.load_component_state_dict); parameter names match this module 1:1, strictly both ways."""
    sd = dict(checkpoint.load_component_state_dict(weight_dir, "unet"))
    own = dict(model.named_parameters())
    for k, v in list(sd.items()):               # SD 1.x: proj_in / proj_out stored as 1x1 convolutions
        if k in own and v.dim() == 4 and own[k].dim() == 2 and v.shape[2:] == (1, 1):
            sd[k] = v[:, :, 0, 0]
    missing, unexpected = model.load_state_dict(sd, strict=False)
    if missing or unexpected:
        raise RuntimeError(f"state dict mismatch: missing {missing[:5]}..., unexpected {unexpected[:5]}...")
    graph.weights_changed()                          # captured graphs of this model (graph.GraphedEpsModel) re-check the parameters before their next replay
    return model


def count_cfg_shared_prefix_flops(model: nn.Module, h: int = 64, w: int = 64) -> int:
    """FLOPs per image of the part of a forward that does not see the context (conv_in, the first resnet, the first transformer's proj_in, self-attention
    and cross-attention query projection): what a cfg_dup forward executes once for two rows of the guidance batch."""
    from torch.utils.flop_counter import FlopCounterMode
    import copy
    m = copy.deepcopy(model).to("meta")
    dt = next(m.parameters()).dtype
    b0 = m.down_blocks[0]
    if b0.attentions is None:
        return 0
    tr = b0.attentions[0]
    blk = tr.transformer_blocks[0]
    x = torch.empty(1, m.conv_in.in_channels, h, w, device="meta", dtype=dt)
    temb = torch.empty(1, m.time_embedding.linear_2.out_features, device="meta", dtype=dt)
    with FlopCounterMode(display=False) as fc:
        hh = m.conv_in(x)
        hh = b0.resnets[0](hh, temb)
        y = tr.proj_in(tr.norm(hh).permute(0, 2, 3, 1).reshape(1, h * w, -1))
        y = y + blk.attn1(blk.norm1(y))
        blk.attn2.to_q(blk.norm2(y))
    return int(fc.get_total_flops())


def count_flops_per_image(model: nn.Module, h: int = 64, w: int = 64, ctx_len: int = 77, ctx_dim: Optional[int] = None) -> int:
    """Forward FLOPs for one image (2 x MACs of conv / linear / attention), via torch's FlopCounterMode on meta tensors.
    (FOLD_FF_OUT changes nothing here: the folded launch's 2 M 5C C FLOPs are those of ff.net[2] and proj_out together.)"""
    from torch.utils.flop_counter import FlopCounterMode
    import copy
    m = copy.deepcopy(model).to("meta")
    if ctx_dim is None:
        ctx_dim = next(mod for n, mod in m.named_modules() if n.endswith("attn2")).to_k.in_features
    dt = next(m.parameters()).dtype
    x = torch.empty(1, 4, h, w, device="meta", dtype=dt)
    t = torch.empty(1, device="meta")
    c = torch.empty(1, ctx_len, ctx_dim, device="meta", dtype=dt)
    with FlopCounterMode(display=False) as fc:
        m(x, t, c)
    return int(fc.get_total_flops())
