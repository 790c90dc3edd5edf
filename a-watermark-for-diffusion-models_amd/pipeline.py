"""End-to-end Gaussian-Shading path on one GPU: embed -> (G1) DDIM or DPM-Solver++ 2M sampling -> (X2) DDIM inversion -> (X3-X5) extract,
everything resident on the device.

Replaces, for the hot path, the reference's per-image flow (extract.py:46-117: `from_pretrained` per image, `.cpu()` of the
inverted latent, scalar Python loops) and the generation loop of modified_stable_diffusion_gs.pyc: the pipeline object is
built once, a batch of independent images moves through the loops together, and nothing returns to the host but
`B x message_length/8` bytes.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import codec
from .ddim import DDIMSchedule, DPMSolverSchedule, ddim_invert_extract, ddim_sample, ddim_invert, dpms_sample

SAMPLERS = ("ddim", "dpmpp_2m", "dpmpp_2m_karras")


class RobustRecordsVote(NamedTuple):
    """What `verify_records(..., robust_levels=L)` returns: (bits, flags, matches) as the other forms, then `codec.RobustVote`'s fields of the last round"""
    bits: torch.Tensor      # uint8 [B, msg_bytes]
    flags: torch.Tensor     # int32 [B]
    matches: torch.Tensor   # int32 [B], recovered bits equal to the record's message
    score: torch.Tensor     # int32 [B, 8 msg_bytes]
    wsum: torch.Tensor      # int32 [B, 8 msg_bytes]
    excess: torch.Tensor    # int32 [B, th, tw]
    wsq: torch.Tensor       # int32 [B, th, tw]
    weights: torch.Tensor   # int32 [B, th, tw]


class GaussianShadingPipeline:
    def __init__(self, eps_model, key: bytes, nonce: bytes, message: bytes, *, height: int = 512, width: int = 512,
                 num_inference_steps: int = 50, dtype: torch.dtype = torch.float16, device="cuda",
                 ctx_uncond: Optional[torch.Tensor] = None, prediction_type: str = "epsilon", l: int = 1,
                 sampler: str = "ddim", num_sampling_steps: Optional[int] = None):
        if sampler not in SAMPLERS:
            raise ValueError(f"unknown sampler {sampler!r}: expected one of " + ", ".join(repr(s) for s in SAMPLERS))
        if hasattr(eps_model, "prepare_context"):          # a unet.UNet2DCondition: small batches replay a captured HIP graph of the forward (graph.py)
            from .graph import graphed
            eps_model = graphed(eps_model, clone_output=False)      # the loops of ddim.py consume eps in the scheduler-step kernel right away
        self.eps_model = eps_model
        self.key, self.nonce, self.message = key, nonce, message
        self.shape = (4, height // 8, width // 8)
        self.dtype, self.device = dtype, torch.device(device)
        self.schedule = DDIMSchedule(num_inference_steps=num_inference_steps, prediction_type=prediction_type)      # inversion / extraction: always DDIM
        # generation: the chosen sampler; None steps = num_inference_steps for DDIM (the same schedule object as before), 20 for DPM-Solver++ 2M
        self.sampler = sampler
        if sampler == "ddim":
            self.sampling_schedule = self.schedule if num_sampling_steps in (None, num_inference_steps) else \
                DDIMSchedule(num_inference_steps=num_sampling_steps, prediction_type=prediction_type)
        else:
            self.sampling_schedule = DPMSolverSchedule(num_inference_steps=20 if num_sampling_steps is None else num_sampling_steps,
                                                       prediction_type=prediction_type, use_karras_sigmas=sampler == "dpmpp_2m_karras")
        self.ctx_uncond = ctx_uncond
        self.message_length = 8 * len(message)
        self.l = codec.check_window(l)                      # cipher bits per lattice element, a property of the deployment like the key

    # E1-E6
    def embed(self, batch: int, *, seed: int = 0, image_index0: int = 0, fast: bool = True, u: Optional[torch.Tensor] = None) -> torch.Tensor:
        return codec.embed_batch(self.key, self.nonce, self.message, batch, self.shape, u=u, seed=seed, image_index0=image_index0,
                                 dtype=self.dtype, fast=fast, device=self.device, l=self.l)

    # E1-E6, one record per image (issue.py): the pipeline's shape, dtype and l, the records' own keys and messages
    def embed_records(self, records: torch.Tensor, msg_bytes: int, *, seed: int = 0, image_index0: int = 0, fast: bool = True,
                      u: Optional[torch.Tensor] = None) -> torch.Tensor:
        return codec.embed_records(records, msg_bytes, self.shape, u=u, seed=seed, image_index0=image_index0, dtype=self.dtype, fast=fast,
                                   l=self.l)

    # X2 + X3-X5 + X6 against each image's own record
    def verify_records(self, x0: torch.Tensor, records: torch.Tensor, msg_bytes: int, *, return_latents: bool = False, soft: bool = False,
                       levels: int = 15, clip: float = 2.5, window_levels: Optional[int] = None, robust_levels: Optional[int] = None, tile: int = 8,
                       iters: int = 2, sign_rounds: int = 1, ecc: Optional[str] = None, ecc_list: int = 1):
        """(bits, flags, matches) of `codec.extract_records` on the DDIM inversion of x0, image b under row b of `records`.
        soft=True: the `codec.SoftVote` (bits, flags, matches, score, wsum, wsq) of `codec.extract_soft` instead, every element weighted by
        one of `levels` reliability levels with thresholds scaled to its image's RMS (`soft.uniform_thresholds(z, levels, clip)`); l = 1 only.
        window_levels=L at the pipeline's l = 2 or 4: the `codec.SoftVote` of `codec.extract_soft_l`, every cipher bit weighted by one of L
        levels (`soft.window_thresholds(z, l, L, clip)`); not with soft=True, and not at l = 1 (that is soft=True).
        robust_levels=L in 1..15, at the pipeline's l: the `RobustRecordsVote` of the one-launch robust decode (`codec.level_pack[_l]` with the
        default table of L levels for this l, then `codec.decode_robust` under each record's own key with `tile`, `iters` and `sign_rounds`;
        matches from `codec.bit_matches` against each record's message); not with soft=True or window_levels.
        ecc="conv": the records' messages are coded payloads (`issue_latents(..., ecc="conv")`); the votes of whichever decoder was chosen go through one
        `codec.viterbi_decode` launch and the result is (what is returned without ecc, `ecc.EccRead`) -- with return_latents (that, EccRead, z).
        ecc_list=2, 4 or 8 with ecc="conv": the list read (`ecc.read_list`), an `ecc.EccListRead` in the EccRead's place; 1 is
        today's launch.  ecc="conv23" / "conv34": the punctured codes through the same two reads."""
        from . import ecc as E
        ecc_list = E.check_list_size(ecc_list)
        if E.check_code(ecc) is not None:
            E.check_length(8 * int(msg_bytes))
        elif ecc_list > 1:
            raise ValueError('ecc_list above 1 needs ecc="conv": the list read is a read of error-corrected payloads')

        def finish(res, z, score):
            if ecc is None:
                return (*res, z) if return_latents else res
            read = E.read_any(score.contiguous(), ecc_list, ecc)
            return (res, read, z) if return_latents else (res, read)

        if robust_levels is not None:
            if soft:
                raise ValueError("robust_levels cannot be combined with soft=True: the robust decode weights by levels AND tiles, in a launch of its own")
            if window_levels is not None:
                raise ValueError("robust_levels cannot be combined with window_levels: the robust decode weights by levels AND tiles, in a launch of its own")
            from . import soft as S
            robust_levels = S._check_table(robust_levels, clip)[0]
            iters = codec._small_int(iters, "iters", 0, codec.ROBUST_MAX_ITERS)
            sign_rounds = codec._small_int(sign_rounds, "sign_rounds", 0, 1)
            if isinstance(tile, bool) or tile not in codec.TILES:
                raise ValueError(f"tile must be one of {codec.TILES} (lattice elements per tile edge), got {tile!r}")
            B, _, msg_bytes = codec._records_operand(records, msg_bytes)
            z = ddim_invert(self.eps_model, x0, self._uncond(x0.shape[0]), self.schedule)
            res = self._robust_records(z, records, B, msg_bytes, robust_levels, clip, tile, iters, sign_rounds)
            return finish(res, z, res.score)
        if soft and self.l != 1:
            raise ValueError(f"soft=True cannot be combined with l = {self.l}: reliability levels are defined for one cipher bit per element")
        if window_levels is not None:
            if soft:
                raise ValueError("window_levels cannot be combined with soft=True: soft=True is the l = 1 form of the vote")
            if self.l == 1:
                raise ValueError("window_levels needs a pipeline with l = 2 or 4: at l = 1 the level-weighted vote is soft=True")
            from . import soft as S
            window_levels = S._check_table(window_levels, clip)[0]
        z = ddim_invert(self.eps_model, x0, self._uncond(x0.shape[0]), self.schedule)
        if window_levels is not None:
            res = codec.extract_soft_l(z, records, msg_bytes, S.window_thresholds(z, self.l, window_levels, clip), self.l)
        elif soft:
            from . import soft as S
            res = codec.extract_soft(z, records, msg_bytes, S.uniform_thresholds(z, levels, clip))
        elif ecc is not None:
            *res, counts = codec.extract_records(z, records, msg_bytes, l=self.l, return_counts=True)
            return finish(tuple(res), z, 2 * counts - codec.vote_copies(z.numel() // z.shape[0], 8 * int(msg_bytes), self.l))
        else:
            res = codec.extract_records(z, records, msg_bytes, l=self.l)
        return finish(res, z, res.score if ecc is not None else None)

    def _robust_records(self, z: torch.Tensor, records: torch.Tensor, B: int, msg_bytes: int, levels: int, clip: float, tile: int, iters: int,
                        sign_rounds: int) -> RobustRecordsVote:
        """`verify_records(robust_levels=...)` after the inversion: one pack launch, one decode launch, the matches per record"""
        from . import soft as S
        if z.dim() != 4 or z.shape[0] != B:
            raise ValueError(f"z must be [{B}, C, h, w] latents, one image per record (got {tuple(z.shape)})")
        z = z.contiguous()
        table = S._default_table(z, self.l, levels, clip)
        rows = codec.level_pack(z, table) if self.l == 1 else codec.level_pack_l(z, table, self.l)
        keys = records[:, :codec.KEYED_RECORD_HEAD].contiguous()
        v = codec.decode_robust(rows.signs, rows.planes, keys, 8 * msg_bytes, tuple(int(s) for s in z.shape[1:]), self.l, tile, iters, sign_rounds)
        msgs = records[:, codec.KEYED_RECORD_HEAD:codec.KEYED_RECORD_HEAD + msg_bytes].cpu().numpy()
        matches = torch.cat([codec.bit_matches(v.bits[b:b + 1].clone(), 8 * msg_bytes, msgs[b].tobytes()) for b in range(B)])
        return RobustRecordsVote(v.bits, rows.flags, matches, v.score, v.wsum, v.excess, v.wsq, v.weights)

    # G1
    def _uncond(self, batch: int) -> torch.Tensor:
        """the empty prompt's context for `batch` images: ONE view object per batch size (the eps model's per-context caches live on the tensor object)"""
        if self.ctx_uncond.shape[0] != 1:
            return self.ctx_uncond
        views = self.__dict__.setdefault("_uncond_views", {})
        ent = views.get(batch)
        if ent is None or ent[0] is not self.ctx_uncond:
            ent = views[batch] = (self.ctx_uncond, self.ctx_uncond.expand(batch, -1, -1))
        return ent[1]

    def generate(self, z_T: torch.Tensor, ctx_text: torch.Tensor, guidance_scale: float = 7.5) -> torch.Tensor:
        cu = self._uncond(z_T.shape[0]) if guidance_scale != 1.0 else None
        sample = ddim_sample if self.sampler == "ddim" else dpms_sample
        return sample(self.eps_model, z_T, ctx_text, self.sampling_schedule, ctx_uncond=cu, guidance_scale=guidance_scale)

    # X2 + X3-X5 (prompt "" -> the unconditional context, guidance 1: extract.py:66-69)
    def invert_and_extract(self, x0: torch.Tensor, *, return_latents: bool = False):
        ctx = self._uncond(x0.shape[0])
        if self.l != 1:                                     # the fused last step votes one bit per element: plain last step, then the l-bit extract
            z = ddim_invert(self.eps_model, x0, ctx, self.schedule)
            res = codec.extract_batch(z, self.key, self.nonce, self.message_length, l=self.l)
            return (*res, z) if return_latents else res
        return ddim_invert_extract(self.eps_model, x0, ctx, self.schedule, self.key, self.nonce, self.message_length,
                                   return_latents=return_latents)

    def invert(self, x0: torch.Tensor) -> torch.Tensor:
        ctx = self._uncond(x0.shape[0])
        return ddim_invert(self.eps_model, x0, ctx, self.schedule)

    def txt2img(self, ctx_text: torch.Tensor, vae, *, latents: Optional[torch.Tensor] = None, seed: int = 0, image_index0: int = 0,
                guidance_scale: float = 7.5):
        """The call of the reference's generation pipeline (`ModifiedStableDiffusionPipeline.__call__` of modified_stable_diffusion_gs.pyc:
        `prepare_latents(latents=Z_s_T)`, keep a copy as `init_latents`, CFG sampling loop, `decode_latents`) with its return order:
        (images [B,3,H,W] in [0,1], has_nsfw_concept = None (no safety checker here), init_latents).  latents=None embeds a fresh Z_s_T batch
        the size of ctx_text."""
        z_T = self.embed(ctx_text.shape[0], seed=seed, image_index0=image_index0) if latents is None else latents.to(self.device, self.dtype)
        init_latents = z_T.clone()
        x0 = self.generate(z_T, ctx_text, guidance_scale)
        return decode_images(x0, vae), None, init_latents

    def roundtrip(self, batch: int, ctx_text: torch.Tensor, *, seed: int = 0, image_index0: int = 0, guidance_scale: float = 7.5):
        z_T = self.embed(batch, seed=seed, image_index0=image_index0)
        x0 = self.generate(z_T, ctx_text, guidance_scale)
        bits, flags = self.invert_and_extract(x0)
        return z_T, x0, bits, flags


# ---------------------------------------------------------------------------------------------------------------------
# image-level stages around the latent loops (X1 / `decode_image`), and the JPEG distortion of BASELINE config 4
# ---------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def decode_images(latents: torch.Tensor, vae) -> torch.Tensor:
    """`decode_image` + `torch_to_numpy` prefix of modified_stable_diffusion_gs.pyc: [B,4,h,w] -> [B,3,8h,8w] in [0,1]."""
    from .vae import latents_to_img
    return latents_to_img(latents, vae)


@torch.no_grad()
def encode_images(images: torch.Tensor, vae) -> torch.Tensor:
    """extract.py:39-43 on a batch already on the device."""
    from .vae import img_to_latents
    return img_to_latents(images, vae)


def jpeg_roundtrip(images: torch.Tensor, quality: int = 10) -> torch.Tensor:
    """JPEG distortion as the reference's `distortions` tool applies it (distortions:175-184: PIL save(quality=QF) / reload) on a
    [B,3,H,W] tensor in [0,1]: quantise to uint8 like numpy_to_pil, run the libjpeg-exact lossy stages on the device
    (imaging.jpeg_roundtrip), return ToTensor values in the input dtype."""
    from . import imaging
    u8 = imaging.tensor_to_image(images)
    return imaging.jpeg_roundtrip(u8, quality, out="f32").to(images.dtype)


def jpeg_roundtrip_pil(images: torch.Tensor, quality: int = 10) -> torch.Tensor:
    """The same through host-side PIL, one image at a time (what the reference does); kept as the checker for the device path."""
    import io
    import numpy as np
    from PIL import Image
    out = []
    for img in (images.detach().float().clamp(0, 1).cpu() * 255).round().to(torch.uint8):
        buf = io.BytesIO()
        Image.fromarray(img.permute(1, 2, 0).numpy()).save(buf, format="JPEG", quality=int(quality))
        buf.seek(0)
        out.append(torch.from_numpy(np.asarray(Image.open(buf).convert("RGB")).copy()).permute(2, 0, 1))
    return (torch.stack(out).float() / 255.0).to(images.device, images.dtype)
