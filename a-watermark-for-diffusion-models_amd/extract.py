"""Drop-in twin of the recover-bits API of the reference's extract.py (extract.py:72-110), with the per-element
norm.cdf loop, the ChaCha20 decrypt and the majority vote running as one HIP kernel.

`args` is the reference's argparse namespace: .key (32 bytes), .nonce (16 bytes), .l (1, 2 or 4 cipher bits per lattice
element; the reference's own l > 1 path is non-functional, SURVEY.md section 5, so l = 2, 4 follow DESIGN.md "Multi-bit windows"),
.message_length.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N
from . import codec

_TORCH_OK = (torch.float16, torch.bfloat16, torch.float32, torch.float64)


def _to_device_latents(reversed_latents, device):
    """np.nditer order (extract.py:82): memory order of the array, i.e. C order for the contiguous tensors the
    inversion returns.  One image per call, any shape."""
    if isinstance(reversed_latents, torch.Tensor):
        t = reversed_latents.detach()
        if t.dtype not in _TORCH_OK:
            t = t.to(torch.float64)
        return t.contiguous().to(device).reshape(1, -1)
    a = np.asarray(reversed_latents)
    if a.dtype not in (np.float16, np.float32, np.float64):
        a = a.astype(np.float64)
    a = np.ascontiguousarray(a.ravel(order="K"))
    return torch.from_numpy(a).to(device).reshape(1, -1)


def _window(args) -> int:
    """args.l as a supported window.  A string or float that counted as l = 1 before windows existed still does (int(l) == 1: a
    namespace built by hand may carry "1" or 1.0); everything else has to be one of codec.WINDOWS as an int."""
    l = getattr(args, "l", 1)
    if isinstance(l, (str, float)) and int(l) == 1:
        return 1
    return codec.check_window(l)


def _soft_wanted(args, l: int) -> bool:
    """--soft as a bool; the combinations the soft vote does not exist for are refused by name"""
    if not int(getattr(args, "soft", 0) or 0):
        return False
    if int(getattr(args, "robust", 0) or 0):
        raise ValueError("--soft 1 cannot be combined with --robust 1: level weights and tile weights are separate votes")
    if l != 1:
        raise ValueError(f"--soft 1 cannot be combined with --l {l}: reliability levels are defined for one cipher bit per element (--l 1)")
    return True


def _window_soft_wanted(args, l: int) -> int:
    """--window_soft L as a number of levels (0: not asked for); the combinations it does not exist for are refused by name"""
    levels = int(getattr(args, "window_soft", 0) or 0)
    if not levels:
        return 0
    if not 1 <= levels <= codec.SOFT_MAX_LEVELS:
        raise ValueError(f"--window_soft takes a number of levels in 1..{codec.SOFT_MAX_LEVELS}, got {levels}")
    for flag in ("soft", "robust"):
        if int(getattr(args, flag, 0) or 0):
            raise ValueError(f"--window_soft cannot be combined with --{flag} 1: it is a vote of its own")
    if getattr(args, "align", None) not in (None, "none"):
        raise ValueError("--window_soft cannot be combined with --align: the alignment search reads the reference's vote")
    if l == 1:
        raise ValueError("--window_soft needs --l 2 or --l 4: at --l 1 the level-weighted vote is --soft 1")
    return levels


def _robust_soft_wanted(args) -> int:
    """--robust_soft L as a number of levels (0: not asked for); it is a decoder of its own and is refused, by name, next to every other one"""
    levels = getattr(args, "robust_soft", 0) or 0
    if not levels:
        return 0
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 1 <= int(levels) <= codec.SOFT_MAX_LEVELS:
        raise ValueError(f"--robust_soft takes a number of levels in 1..{codec.SOFT_MAX_LEVELS}, got {levels!r}")
    for flag in ("soft", "robust"):
        if int(getattr(args, flag, 0) or 0):
            raise ValueError(f"--robust_soft cannot be combined with --{flag} 1: it weights by levels AND tiles, in a decoder of its own")
    if int(getattr(args, "window_soft", 0) or 0):
        raise ValueError("--robust_soft cannot be combined with --window_soft: it weights by levels AND tiles, in a decoder of its own")
    if getattr(args, "align", None) not in (None, "none"):
        raise ValueError("--robust_soft cannot be combined with --align: the alignment search reads the reference's vote")
    return int(levels)


class _AlignedBits(str):
    """A recovered bit string that also says under which alignment of the lattice it was read (--align)"""
    alignment = None
    log10_p = 0.0


def _align_wanted(args) -> bool:
    """--align flips|d4 as a bool; the votes it does not exist for are refused by name"""
    if getattr(args, "align", None) in (None, "none"):
        return False
    for flag in ("soft", "robust"):
        if int(getattr(args, flag, 0) or 0):
            raise ValueError(f"--align cannot be combined with --{flag} 1: the alignment search reads the reference's vote")
    if int(getattr(args, "window_soft", 0) or 0):
        raise ValueError("--window_soft cannot be combined with --align: the alignment search reads the reference's vote")
    if getattr(args, "tamper_map", None):
        raise ValueError("--align cannot be combined with --tamper_map")
    return True


def _vote_aligned(z, args, m: int, l: int):
    """--align: `align.extract_aligned` under the run's key -> (one _AlignedBits or ValueError per image)"""
    from . import align as AL
    if z.dim() != 4:
        raise ValueError(f"--align needs the latents as [B, C, h, w] (got {tuple(z.shape)})")
    cands = AL.alignments(args.align, int(getattr(args, "align_shift", 0) or 0), z.shape[-2], z.shape[-1])
    out = []
    for r in AL.extract_aligned(z, args.key, args.nonce, m, cands, l=l):
        if r.flags & N.GSW_FLAG_NAN:
            out.append(ValueError("cannot convert float NaN to integer"))
        elif r.flags & N.GSW_FLAG_SATURATED:
            out.append(ValueError("invalid literal for int() with base 2"))
        else:
            s = _AlignedBits(codec.bits_to_str(r.bits)[:m])
            s.alignment, s.log10_p = r.alignment, r.log10_p
            out.append(s)
    return out


def _alignment_note(r) -> str:
    """what --align adds to an image's line: the alignment it was read under and its bound over the candidates"""
    from . import align as AL
    return f", alignment: {AL.describe(r.alignment)}, log10 p, {r.log10_p:.3f}" if isinstance(r, _AlignedBits) else ""


class _EccBits(str):
    """A recovered bit string (the vote's, as without --ecc) that also carries the payload read of the same votes (--ecc conv)"""
    note = ""


def _ecc_wanted(args):
    """--ecc as None or a code of `ecc.CODES`; next to --align, --align_shift or several GPUs it is refused by name, and the message length must be a coded one"""
    code = getattr(args, "ecc", None)
    if code is None:
        if _ecc_list(args) > 1:
            raise ValueError("--ecc_list above 1 needs --ecc conv: the list read is a read of error-corrected payloads")
        return None
    from . import ecc as E
    E.check_code(code)
    E.check_list_size(_ecc_list(args))
    for flag, on in (("--align", getattr(args, "align", None) not in (None, "none")), ("--align_shift", bool(int(getattr(args, "align_shift", 0) or 0)))):
        if on:
            raise ValueError(f"--ecc cannot be combined with {flag} yet: the payload read is not wired through the alignment search")
    if int(getattr(args, "gpus", 1) or 1) > 1:
        raise ValueError("--ecc cannot be combined with --gpus above 1 yet: the payload read runs on one GPU")
    E.check_length(int(args.message_length))
    return code


def _ecc_list(args) -> int:
    """--ecc_list: the list size of the payload read, 1 (the plain read) when absent"""
    v = getattr(args, "ecc_list", 1)
    return 1 if v is None else v


def _ecc_note(r) -> str:
    """what --ecc adds after an image's line"""
    return f"\n{r.note}" if isinstance(r, _EccBits) and r.note else ""


def _with_payloads(strings, score, m: int, list_size: int = 1, code: str = "conv"):
    """the bit strings of a batch (or the exceptions raised for them) -> the same, every string carrying its payload read: ONE `ecc.read` launch, with
    --ecc_list above 1 ONE `ecc.read_list` launch"""
    from . import ecc as E
    read = E.read_any(score.contiguous(), list_size, code)
    out = []
    for b, s in enumerate(strings):
        if not isinstance(s, Exception):
            s = _EccBits(s)
            s.note = E.format_any(read, b, m, list_size, code)
        out.append(s)
    return out


def _vote(z, args, m: int, l: int):
    return _vote_scored(z, args, m, l, False)[:2]


def _vote_scored(z, args, m: int, l: int, want_score: bool = True):
    """(bits, flags, score) of the reference's vote, with --robust 1 of the tile-weighted vote (tamper.extract_robust, its default iterations), with
    --soft 1 of the level-weighted vote (soft.extract_soft, thresholds scaled to each image's RMS), with --window_soft L at --l 2 / 4 of the
    vote with a level per cipher bit (soft.extract_soft_l, soft.window_thresholds), with --robust_soft L of the robust decode with levels
    (tamper.extract_robust_soft: --tile, --iters, --sign_rounds, at any --l).  score: the int32 [B, m] votes the bits are the signs of (the plain vote's
    2 counts - copies, asked for with want_score only: without it the launch is the one it always was)"""
    robust_levels = _robust_soft_wanted(args)
    if robust_levels:
        from . import tamper
        res = tamper.extract_robust_soft(z, args.key, args.nonce, m, l=l, tile=int(getattr(args, "tile", 8)), iters=int(getattr(args, "iters", 2)),
                                         levels=robust_levels, clip=float(getattr(args, "soft_clip", 2.5)), sign_rounds=int(getattr(args, "sign_rounds", 1)))
        return res.bits, res.flags, res.score
    window_levels = _window_soft_wanted(args, l)
    if window_levels:
        from . import soft
        res = soft.extract_soft_l(z, args.key, args.nonce, m, l, levels=window_levels, clip=float(getattr(args, "soft_clip", 2.5)))
        return res.bits, res.flags, res.score
    if _soft_wanted(args, l):
        from . import soft
        res = soft.extract_soft(z, args.key, args.nonce, m, levels=int(getattr(args, "soft_levels", 15)), clip=float(getattr(args, "soft_clip", 2.5)))
        return res.bits, res.flags, res.score
    if int(getattr(args, "robust", 0) or 0):
        from . import tamper
        return tamper.extract_robust(z, args.key, args.nonce, m, l=l, tile=int(getattr(args, "tile", 8)))[:3]
    if not want_score:
        return codec.extract_batch(z, args.key, args.nonce, m, l=l) + (None,)
    bits, flags, counts = codec.extract_batch(z, args.key, args.nonce, m, return_counts=True, l=l)
    return bits, flags, 2 * counts - codec.vote_copies(z.numel() // z.shape[0], m, l)


def write_tamper_maps(latents, files, args) -> None:
    """--tamper_map DIR: the map of every image against --original_message_hex (a message known independently of the image), written as
    DIR/<image>.tamper.npy / .tamper.png; an image whose latents the reference rejects writes nothing (its error is the vote's to report)."""
    from . import tamper
    maps = tamper.tamper_map(latents, args.key, args.nonce, bytes.fromhex(args.original_message_hex), l=_window(args), tile=int(args.tile),
                             message_length=int(args.message_length))
    for f, tm in zip(files, maps):
        if not isinstance(tm, Exception):
            tamper.save_map(tm, tamper.map_stem(args.tamper_map, f), (args.width, args.height))


def recover_exactracted_message(reversed_latents, args, *, device="cuda"):
    """extract.py:72-101 -> str of message_length '0'/'1' characters.

    Raises ValueError where the reference does (a latent >= 8.2924 saturates norm.cdf so int(y) == 2, or NaN;
    extract.py:84-86) and IndexError when the padded bit count is not a multiple of message_length (extract.py:98).
    """
    l = _window(args)
    z = _to_device_latents(reversed_latents, device)
    m = int(args.message_length)
    robust_soft = _robust_soft_wanted(args)
    code = _ecc_wanted(args)
    if _align_wanted(args):                                  # the alignments act on the lattice: the search needs the image's [C, h, w]
        shape = tuple(int(d) for d in np.shape(reversed_latents))
        if len(shape) < 3 or int(np.prod(shape[-3:])) != z.numel():
            raise ValueError(f"--align needs the latents of ONE image as [..., C, h, w] (got {shape})")
        r = _vote_aligned(z.view(1, *shape[-3:]), args, m, l)[0]
        if isinstance(r, Exception):
            raise r
        return r
    if robust_soft or int(getattr(args, "robust", 0) or 0):  # the tiles are cut from the lattice: the weighted vote needs the image's [C, h, w]
        shape = tuple(int(d) for d in np.shape(reversed_latents))
        if len(shape) < 3 or int(np.prod(shape[-3:])) != z.numel():
            raise ValueError(f"{'--robust_soft' if robust_soft else '--robust 1'} needs the latents of ONE image as [..., C, h, w] (got {shape})")
        z = z.view(1, *shape[-3:])
    bits, flags, score = _vote_scored(z, args, m, l, code is not None)
    f = int(flags[0].item())
    if f & N.GSW_FLAG_NAN:
        raise ValueError("cannot convert float NaN to integer")
    if f & N.GSW_FLAG_SATURATED:
        raise ValueError("invalid literal for int() with base 2")
    text = codec.bits_to_str(bits[0].cpu().numpy())[:m]
    return text if code is None else _with_payloads([text], score[:1], m, _ecc_list(args), code)[0]


def recover_exactracted_message_batch(latents: torch.Tensor, args):
    """Batch form: latents [B, 4, h, w] on the device -> (list of bit strings or the raised exception per image).
    Mirrors the per-image try/except of extract.py:148-155."""
    l = _window(args)
    m = int(args.message_length)
    _robust_soft_wanted(args)
    code = _ecc_wanted(args)
    if _align_wanted(args):
        return _vote_aligned(latents.contiguous(), args, m, l)
    bits, flags, score = _vote_scored(latents.contiguous(), args, m, l, code is not None)
    bits_h, flags_h = bits.cpu().numpy(), flags.cpu().numpy()
    out = []
    for b in range(bits_h.shape[0]):
        if flags_h[b] & N.GSW_FLAG_NAN:
            out.append(ValueError("cannot convert float NaN to integer"))
        elif flags_h[b] & N.GSW_FLAG_SATURATED:
            out.append(ValueError("invalid literal for int() with base 2"))
        else:
            out.append(codec.bits_to_str(bits_h[b])[:m])
    return out if code is None else _with_payloads(out, score, m, _ecc_list(args), code)


def calculate_bit_accuracy(original_message_hex, extracted_message_bin):
    """Host twin of extract.py:103-110: (the key's bits as a '0'/'1' string cut to the common length, fraction of positions that agree).  The hex string
    becomes 4 bits per digit, MSB first, leading zeros kept; the shorter of the two strings bounds
    the comparison; an empty comparison divides by zero like the reference does.  The batched device form is codec.bit_matches."""
    width = 4 * len(original_message_hex)                           # four bits per hex digit, leading zeros kept
    want = format(int(original_message_hex, 16), "b").zfill(width)  # (ValueError for a non-hex string, like the reference)
    n = min(len(want), len(extracted_message_bin))
    want = want[:n]
    agree = sum(a == b for a, b in zip(want, extracted_message_bin))
    return want, agree / n


# =====================================================================================================================
# X1 + X2 + H1: the rest of extract.py -- image -> latents -> DDIM inversion, the per-image / per-directory harness and
# the CLI.  Same function names, `args` fields, stdout / result.txt text as the reference (extract.py:23-70,112-211).
# Differences that are the point of the build: the models are loaded ONCE (the reference calls from_pretrained per image,
# extract.py:56-60), the images of ALL directories of a run go through the UNet loop in full device batches, and the inverted
# latents stay on the device for the vote (the reference returns `.cpu()`, extract.py:70).
# =====================================================================================================================
import glob
import os
import sys
from datetime import datetime

_MODEL_CACHE = {}

# Results are only meaningful with real checkpoint weights.  When `model_id` is not a local diffusers directory (the reference's default hub
# id cannot be downloaded here) the harness REFUSES to run unless synthetic weights are allowed explicitly: this switch, the environment
# variable GSW_ALLOW_SYNTHETIC_WEIGHTS=1 or the CLI flag --allow_synthetic_weights (bench and tests set it; every result file then carries
# a SYNTHETIC WEIGHTS marker and no roll-up line is written).
ALLOW_SYNTHETIC_WEIGHTS = False


def _synthetic_allowed(args=None) -> bool:
    return bool(ALLOW_SYNTHETIC_WEIGHTS or os.environ.get("GSW_ALLOW_SYNTHETIC_WEIGHTS", "0") == "1" or (args is not None and getattr(args, "allow_synthetic_weights", False)))


def _no_checkpoint(model_id) -> bool:
    """True when `model_id` resolves to no local checkpoint (neither a directory nor a cached hub snapshot): synthetic weights or failure"""
    from .checkpoint import resolve_model_dir
    return resolve_model_dir(str(model_id)) is None


def _read_json(path):
    import json
    with open(path) as f:
        return json.load(f)


def _unet_from_config(cfg: dict):
    """unet/config.json (diffusers UNet2DConditionModel) -> the own module.  `attention_head_dim` is the number of heads in the SD 1.x /
    2.x configs (an int or one entry per block); head width = channels / heads."""
    from . import unet as U
    from .checkpoint import validate_unet_config
    validate_unet_config(cfg)
    boc = tuple(cfg.get("block_out_channels", (320, 640, 1280, 1280)))
    ahd = cfg.get("attention_head_dim", 8)
    heads = tuple(ahd) if isinstance(ahd, (list, tuple)) else (int(ahd),) * len(boc)
    down = cfg.get("down_block_types", ["CrossAttnDownBlock2D"] * (len(boc) - 1) + ["DownBlock2D"])
    for k, want in (("layers_per_block", 2), ("norm_num_groups", 32), ("act_fn", "silu"), ("center_input_sample", False), ("flip_sin_to_cos", True), ("freq_shift", 0)):
        if cfg.get(k, want) != want:
            raise ValueError(f"unet/config.json: {k}={cfg[k]!r} is not supported (expected {want!r})")
    return U.UNet2DCondition(in_channels=int(cfg.get("in_channels", 4)), out_channels=int(cfg.get("out_channels", 4)), block_out_channels=boc,
                             layers_per_block=2, cross_attention_dim=int(cfg.get("cross_attention_dim", 1024)), num_heads=heads, head_dim=None,
                             attn_blocks=tuple(t.startswith("CrossAttn") for t in down))


def _vae_from_config(cfg: dict):
    from . import vae as V
    if cfg.get("layers_per_block", 2) != 2 or cfg.get("norm_num_groups", 32) != 32:
        raise ValueError("vae/config.json: only layers_per_block 2 / 32 norm groups (the SD autoencoder) are supported")
    return V.AutoencoderKL(block_out_channels=tuple(cfg.get("block_out_channels", (128, 256, 512, 512))), latent_channels=int(cfg.get("latent_channels", 4)))


class Models:
    """UNet + VAE + scheduler constants + the context of the empty prompt of one `model_id`: a local directory in diffusers layout (unet/,
    vae/, scheduler/, text_encoder/ + tokenizer/) or a hub id such as the reference's default `stabilityai/stable-diffusion-2-1-base`
    (extract.py:183), which is looked up in the local Hugging Face cache exactly where diffusers' from_pretrained (extract.py:56-60) would have
    left it (checkpoint.resolve_model_dir; nothing is ever downloaded).  The modules are built from the directory's config.json files, so SD 1.x
    and 2.x checkpoints both load; safetensors, sharded safetensors and .bin weight files are read."""

    def __init__(self, model_id, device="cuda", dtype=torch.float16, allow_synthetic=False):
        from . import unet as U, vae as V, checkpoint
        self.device, self.dtype, self.model_name = torch.device(device), dtype, str(model_id)
        resolved = checkpoint.resolve_model_dir(self.model_name)
        self.synthetic = resolved is None
        self.model_id = self.model_name if resolved is None else resolved        # from here on: the directory the files are read from
        self.scheduler = {}
        if self.synthetic:
            if not allow_synthetic:
                raise FileNotFoundError(
                    f"'{model_id}' is neither a local directory in diffusers layout nor a snapshot in the local Hugging Face cache (searched: "
                    f"{checkpoint.describe_search(self.model_name)}), and there is no network to fetch it from. Pass a checkpoint directory as "
                    "--model_id; for pipeline tests / benchmarks with seeded SYNTHETIC weights (bit accuracies are then meaningless) opt in with "
                    "--allow_synthetic_weights, GSW_ALLOW_SYNTHETIC_WEIGHTS=1 or extract.ALLOW_SYNTHETIC_WEIGHTS = True.")
            print(f"[gswm] '{model_id}' is not a local diffusers directory: SYNTHETIC weights (results are not meaningful)", file=sys.stderr)
            self.unet = U.synthetic_init_(U.UNet2DCondition(), 0)
            self.vae = V.synthetic_init_(V.AutoencoderKL(), 1)
        else:
            ucfg = os.path.join(self.model_id, "unet", "config.json")
            vcfg = os.path.join(self.model_id, "vae", "config.json")
            self.unet = _unet_from_config(_read_json(ucfg)) if os.path.exists(ucfg) else U.UNet2DCondition()
            self.vae = _vae_from_config(_read_json(vcfg)) if os.path.exists(vcfg) else V.AutoencoderKL()
            U.load_diffusers_state_dict(self.unet, self.model_id)
            V.load_diffusers_state_dict(self.vae, self.model_id)
            scfg = os.path.join(self.model_id, "scheduler", "scheduler_config.json")
            if os.path.exists(scfg):
                self.scheduler = _read_json(scfg)
                checkpoint.validate_scheduler_config(self.scheduler)
        self.unet.num_train_timesteps = int(self.scheduler.get("num_train_timesteps", 1000)) if self.scheduler else 1000      # length of the time-embedding table (unet.TEMB_TABLE)
        self.unet.to(self.device, dtype).eval()
        self.vae.to(self.device, dtype).eval()
        from .graph import graphed
        self.eps = graphed(self.unet, clone_output=False)           # the eps model of the loops: HIP-graph replay of the forward for small batches (graph.py), eager above
        self.prediction_type = self.scheduler.get("prediction_type", "epsilon")
        self.ctx_dim = self.unet.mid_block.attentions[0].transformer_blocks[0].attn2.to_k.in_features
        self.ctx_empty = self._empty_prompt_context()

    def schedule_kwargs(self) -> dict:
        """DDIM constants of scheduler/scheduler_config.json (defaults = the SD config)."""
        c = self.scheduler
        if c and c.get("beta_schedule", "scaled_linear") != "scaled_linear":
            raise ValueError(f"scheduler_config.json: beta_schedule {c['beta_schedule']!r} is not supported")
        return dict(num_train_timesteps=int(c.get("num_train_timesteps", 1000)), steps_offset=int(c.get("steps_offset", 1)),
                    set_alpha_to_one=bool(c.get("set_alpha_to_one", False)), beta_start=float(c.get("beta_start", 0.00085)),
                    beta_end=float(c.get("beta_end", 0.012)))

    def _empty_prompt_context(self):
        """Context of prompt "" (extract.py:66): the CLIP text encoder of the directory (text.py), else -- synthetic weights only -- a fixed
        seeded tensor of the right shape."""
        te = os.path.join(self.model_id, "text_encoder")
        if not self.synthetic and os.path.isdir(te):
            from . import text
            return text.encode_prompt_from_dir(self.model_id, [""], self.device, self.dtype)
        if not self.synthetic:
            raise FileNotFoundError(f"{te} is missing: the inversion needs the context of the empty prompt (extract.py:66)")
        g = torch.Generator().manual_seed(77)
        return torch.randn(1, 77, self.ctx_dim, generator=g).to(self.device, self.dtype)


def load_models(model_id, device="cuda", dtype=torch.float16, allow_synthetic=None) -> Models:
    allow = _synthetic_allowed() if allow_synthetic is None else bool(allow_synthetic)
    k = (str(model_id), str(device), dtype)
    m = _MODEL_CACHE.get(k)
    if m is not None and m.synthetic and not allow:
        # a synthetic model cached by an earlier opt-in call must not be handed to a fail-closed one
        raise FileNotFoundError(f"'{model_id}' is not a local checkpoint directory and synthetic weights are not allowed for this call "
                                "(a synthetic model of that name is cached from an earlier, explicitly allowed call)")
    if m is None:
        m = _MODEL_CACHE[k] = Models(model_id, device, dtype, allow_synthetic=allow)
    return m


def load_image(imgname, target_size=None) -> torch.Tensor:
    """extract.py:31-37: PIL RGB, optional Lanczos resize to (w, h), ToTensor -> float32 [1,3,H,W] in [0,1]."""
    from PIL import Image
    pil_img = Image.open(imgname).convert("RGB")
    if target_size is not None:
        if isinstance(target_size, int):
            target_size = (target_size, target_size)
        pil_img = pil_img.resize(tuple(target_size), Image.Resampling.LANCZOS)
    a = np.asarray(pil_img, dtype=np.uint8)
    return torch.from_numpy(a.copy()).permute(2, 0, 1).float().div_(255.0)[None]


def decode_image_file(path) -> np.ndarray:
    """Host side of load_image: file -> uint8 [H, W, 3] (PIL decode + RGB conversion, extract.py:32)."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8).copy()


def images_to_device(arrs, target_size=None, *, device="cuda", out="f16") -> torch.Tensor:
    """uint8 images -> the tensor `load_image(...).to(float16)` / `2.*x - 1.` produce (extract.py:31-37,48,40), resized and normalised on
    the device (imaging.resize_lanczos, bit-identical to the PIL / torchvision chain).  Images of one call must share a size after resizing
    (they do in the reference's use: --width / --height)."""
    from . import imaging
    if isinstance(target_size, int):
        target_size = (target_size, target_size)
    groups = {}
    for i, a in enumerate(arrs):
        groups.setdefault(a.shape, []).append(i)
    outs = [None] * len(arrs)
    for shape, idx in groups.items():
        dev = torch.from_numpy(np.stack([arrs[i] for i in idx])).to(device)
        res = imaging.resize_lanczos(dev, None if target_size is None else tuple(target_size), out=out)
        for j, i in enumerate(idx):
            outs[i] = res[j]
    if len({tuple(o.shape) for o in outs}) != 1:
        raise ValueError("images of one batch must have one size after resizing (pass target_size)")
    return torch.stack(outs)


def load_images_device(image_paths, target_size=None, *, device="cuda", out="f16") -> torch.Tensor:
    """Batch form of load_image + normalisation: file decoding on the host, everything else on the device."""
    return images_to_device([decode_image_file(p) for p in image_paths], target_size, device=device, out=out)


def img_to_latents(x: torch.Tensor, vae):
    """extract.py:39-43."""
    from . import vae as V
    return V.img_to_latents(x, vae)


def _scheduler_steps(args, models):
    from .ddim import DDIMSchedule
    kw = models.schedule_kwargs() if hasattr(models, "schedule_kwargs") else {}
    if args.scheduler == "DDIM":
        return DDIMSchedule(num_inference_steps=int(args.num_inference_steps), prediction_type=models.prediction_type, **kw)
    if args.scheduler == "DPMs":
        from .ddim import DPMSolverInverseSchedule
        return DPMSolverInverseSchedule(num_inference_steps=int(args.num_inference_steps), prediction_type=models.prediction_type)
    raise ValueError("Please choose 'DPMs' or 'DDIM' for the scheduler.")     # extract.py:54


@torch.no_grad()
def invert_decoded_images(arrs, args, *, device="cuda") -> torch.Tensor:
    """uint8 RGB images -> [B,4,h,w] inverted latents on the DEVICE (resize, normalise, VAE encode, DDIM / DPM-Solver++ inversion)."""
    from .ddim import ddim_invert, dpms_invert, DPMSolverInverseSchedule
    from . import vae as V
    models = load_models(args.model_id, device, allow_synthetic=_synthetic_allowed(args))
    sched = _scheduler_steps(args, models)
    if models.dtype == torch.float16:
        xn = images_to_device(arrs, [args.width, args.height], device=models.device, out="f16")      # = 2 * fp16(ToTensor) - 1
    else:
        xn = 2.0 * images_to_device(arrs, [args.width, args.height], device=models.device, out="f32").to(models.dtype) - 1.0
    latents = V.normalised_img_to_latents(xn, models.vae)
    ctx = models.ctx_empty.expand(latents.shape[0], -1, -1)
    if isinstance(sched, DPMSolverInverseSchedule):
        return dpms_invert(models.eps, latents, ctx, sched)
    return ddim_invert(models.eps, latents, ctx, sched)


def exactract_latents_batch(image_paths, args, *, device="cuda") -> torch.Tensor:
    """Batch form of exactract_latents: [B,4,h,w] fp16 latents on the DEVICE."""
    return invert_decoded_images([decode_image_file(p) for p in image_paths], args, device=device)


def exactract_latents(args, *, device="cuda") -> torch.Tensor:
    """extract.py:46-70 -> fp16 CPU tensor [1,4,h,w] like the reference (use exactract_latents_batch to stay on the device)."""
    return exactract_latents_batch([args.single_image_path], args, device=device).cpu()


def get_result_for_one_image(args):
    """extract.py:112-117 (same stdout text)."""
    if _no_checkpoint(args.model_id):
        load_models(args.model_id, allow_synthetic=_synthetic_allowed(args))
        print(f"{SYNTHETIC_MARKER}: '{args.model_id}' is not a local checkpoint, the bit accuracy below is not meaningful", file=sys.stderr)
    reversed_latents = exactract_latents_batch([args.single_image_path], args)
    if getattr(args, "tamper_map", None):
        write_tamper_maps(reversed_latents, [args.single_image_path], args)
    extracted_message_bin = recover_exactracted_message(reversed_latents, args)
    original_message_bin, bit_accuracy = calculate_bit_accuracy(args.original_message_hex, extracted_message_bin)
    print(f"{os.path.basename(args.single_image_path)}\nOriginal Message: {original_message_bin} \nExtracted Message: {extracted_message_bin}\n"
          f"Bit Accuracy: {bit_accuracy}{_alignment_note(extracted_message_bin)}{_ecc_note(extracted_message_bin)}\n")
    return original_message_bin, extracted_message_bin, bit_accuracy


def write_batch_info(result_file, args):
    """The header block of a result.txt (wire format of extract.py:165-175)."""
    bar = "=" * 40
    stamp = datetime.now().strftime("%Y-%m-%d %H:%M:%S")
    fields = [("Time", stamp)] + [(k, getattr(args, k)) for k in ("key_hex", "nonce_hex", "original_message_hex", "num_inference_steps", "scheduler")]
    result_file.write(f"{bar}Batch Info{bar}\n" + "".join(f"{k},{v}\n" for k, v in fields) + f"{bar}Batch Start{bar}\n")


SYNTHETIC_MARKER = "SYNTHETIC WEIGHTS"
UNPINNED_MARKER = "PARITY UNPINNED"


class _DirJob:
    """One directory of the run: its image files in the reference's order (*.png then *.jpg, extract.py:135) and, after the device pass,
    one outcome per file -- the recovered bit string or the exception that file raised."""

    def __init__(self, path):
        self.path = path
        self.files = glob.glob(os.path.join(path, "*.png")) + glob.glob(os.path.join(path, "*.jpg"))
        self.outcome = {}


def _plan(args):
    """The run as a flat script: ("banner", dir) / ("job", _DirJob) entries in the order the reference visits directories
    (extract.py:120-132: every sub-directory of every os.walk level, or just the one directory)."""
    script = []
    if int(args.is_traverse_subdirectories) == 1:
        for here, subdirs, _ in os.walk(args.images_directory_path):
            script.append(("banner", here))
            script += [("job", _DirJob(os.path.join(here, d))) for d in subdirs]
    else:
        script.append(("job", _DirJob(args.images_directory_path)))
    return script


class _RemoteError(Exception):
    """An exception raised for one image on another rank: only its text travels (the result files hold `str(e)`)."""


DECODE_WINDOW_BATCHES = 2      # host-decoded images held at a time = this many device batches per rank (bounds host memory on large trees)


def _recover_items(items, args, batch_size, pool=None):
    """items: [file] -> [outcome] (the recovered bit string or the exception that file raised), in order.  Decode the files on the host
    (a file that does not decode fails alone), push the decodable ones through resize -> VAE -> inversion -> vote in full device batches;
    if a batch raises, its images are redone one by one so that each reports its own error, like the reference's per-image try / except
    (extract.py:148-155).  The decoded arrays die with this call."""
    def decode(f):
        try:
            return decode_image_file(f)
        except Exception as e:                      # a file that does not decode fails alone
            return e

    decoded = list(pool.map(decode, items)) if pool is not None else [decode(f) for f in items]
    out = list(decoded)
    ready = [i for i, r in enumerate(decoded) if not isinstance(r, Exception)]

    def run(idx):
        latents = invert_decoded_images([decoded[i] for i in idx], args)
        if getattr(args, "tamper_map", None):
            write_tamper_maps(latents, [items[i] for i in idx], args)
        return recover_exactracted_message_batch(latents, args)

    for k in range(0, len(ready), batch_size):
        idx = ready[k:k + batch_size]
        try:
            results = run(idx)
        except Exception:
            results = []
            for i in idx:
                try:
                    results += run([i])
                except Exception as e:
                    results.append(e)
        for i, r in zip(idx, results):
            out[i] = r
    return out


def _recover_many(items, args, batch_size, on_window=None):
    """items: [(job, file)] across ALL directories, in plan order.  The run is cut into WINDOWS of world x DECODE_WINDOW_BATCHES x batch_size
    images: inside a window rank r takes the contiguous slice dist.shard_range gives it (images are independent: no collective on the data
    path), the outcomes of the window are all-gathered as text, and every rank records them -- so at most a window's worth of decoded
    images is alive per process, and `on_window()` (rank 0: flush the result files of every directory that is now complete) runs as the
    work proceeds.  One process: the same loop with world = 1."""
    from . import dist as gdist
    from concurrent.futures import ThreadPoolExecutor
    rank, world = gdist.rank_world()
    window = world * DECODE_WINDOW_BATCHES * batch_size
    # PIL releases the GIL while it reads and decodes: a few host threads keep the device batches fed on large directories
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        for w0 in range(0, len(items), window):
            win = items[w0:w0 + window]
            lo, hi = gdist.shard_range(len(win), rank, world)
            mine = _recover_items([f for _, f in win[lo:hi]], args, batch_size, pool)
            if world > 1:
                wire = [("err", f"{r}") if isinstance(r, Exception) else ("ok", r) for r in mine]
                parts = gdist.gather_objects(wire)
                flat = [x for part in parts for x in part]
                outcomes = [_RemoteError(v) if k == "err" else v for k, v in flat]
            else:
                outcomes = mine
            for (job, f), r in zip(win, outcomes):
                job.outcome[f] = r
            if on_window is not None:
                on_window()


def _report(job, args, synthetic):
    """Write one directory's result.txt block (+ the roll-up line in its parent) and echo the per-image text, byte for byte the
    reference's (extract.py:112-117,139-163).  With synthetic weights (or the parity-unpinned DPM-Solver++ scheduler) a marker line
    follows the header; no roll-up is written with synthetic weights."""
    if not job.files:
        return
    accs = []
    with open(os.path.join(job.path, "result.txt"), "a") as out:
        write_batch_info(out, args)
        if synthetic:
            out.write(f"{SYNTHETIC_MARKER},'{args.model_id}' is not a local checkpoint: the bit accuracies below are not meaningful\n")
        if str(getattr(args, "scheduler", "DDIM")) == "DPMs":
            out.write(f"{UNPINNED_MARKER},--scheduler DPMs restates DPM-Solver++ (2M) from the paper: diffusers' DPMSolverMultistepInverseScheduler "
                      "(extract.py:49-50) could not be executed to pin it; --scheduler DDIM is pinned against the reference\n")
        for f in job.files:
            r = job.outcome.get(f, RuntimeError("not processed"))
            if isinstance(r, Exception):
                print(f"Error processing {f}: {r}\n")
                out.write(f"Error processing {f}: {r}\n")
                continue
            original_message_bin, bit_accuracy = calculate_bit_accuracy(args.original_message_hex, r)
            name = os.path.basename(f)
            print(f"{name}\nOriginal Message: {original_message_bin} \nExtracted Message: {r}\nBit Accuracy: {bit_accuracy}{_alignment_note(r)}{_ecc_note(r)}\n")
            out.write(f"{name}, Bit Accuracy, {bit_accuracy}{_alignment_note(r)}\n")
            if _ecc_note(r):
                out.write(f"{name}, {r.note}\n")
            accs.append(float(bit_accuracy))
        if accs:
            mean = sum(accs) / len(accs)
            out.write(f"Average Bit Accuracy, {mean}\n\n" + "=" * 40 + "Batch End" + "=" * 40 + "\n")
    if accs and not synthetic:
        with open(os.path.join(os.path.dirname(job.path), "result.txt"), "a") as up:
            up.write(f"{os.path.basename(job.path)}, Average Bit Accuracy, {mean}\n")


class _Reporter:
    """Replays the plan in the reference's order as directories complete: a directory's block is written as soon as every image of it
    AND of every directory before it has an outcome (so a crash mid-run leaves the finished directories' result.txt behind, like the
    reference's append-as-you-go loop, extract.py:143-155, and stdout / roll-up lines keep the reference's order)."""

    def __init__(self, script, args, synthetic):
        self.script, self.args, self.synthetic, self.pos = script, args, synthetic, 0

    def flush(self):
        while self.pos < len(self.script):
            kind, x = self.script[self.pos]
            if kind == "banner":
                print("=" * 20 + x + "=" * 20)
            else:
                if any(f not in x.outcome for f in x.files):
                    return
                _report(x, self.args, self.synthetic)
            self.pos += 1


import contextlib


@contextlib.contextmanager
def _strictness(args, synthetic):
    """--strict_kernels: a half-precision GPU call that would leave the hand-written kernels (a checkpoint whose shapes miss the engine's
    K % 64 / N % 8 grid, an odd lattice) raises instead of warning.  Default: ON (round 6: also with synthetic weights -- a silent change of backend is
    not a behaviour to discover from a warning); `--strict_kernels 0` opts into the library kernels.  Scoped to the harness call: the previous setting is
    restored on the way out."""
    from . import unet as U, vae as V
    want = getattr(args, "strict_kernels", None)
    strict = True if want is None else bool(int(want))
    before = (U.STRICT, V.STRICT)
    U.STRICT = V.STRICT = strict
    try:
        yield strict
    finally:
        U.STRICT, V.STRICT = before


def process_directory(args, *, batch_size=None):
    """The directory harness (extract.py:120-163) in batch form: plan the whole run, recover the images of every directory in full device
    batches -- sharded over the ranks of the process group when there is one (`--gpus N`), streamed in bounded windows -- and write the
    result files in the reference's order and format as the directories complete (rank 0 writes; the other ranks stay silent)."""
    from . import dist as gdist
    batch_size = int(batch_size or getattr(args, "batch_size", 0) or 16)
    rank, _ = gdist.rank_world()
    script = _plan(args)
    jobs = [j for kind, j in script if kind == "job"]
    synthetic = _no_checkpoint(args.model_id)
    with _strictness(args, synthetic):
        if any(j.files for j in jobs):
            load_models(args.model_id, allow_synthetic=_synthetic_allowed(args))          # fail before touching any result file
        traverse = int(args.is_traverse_subdirectories) == 1
        writer = rank == 0
        if traverse and writer:
            with open(os.path.join(args.images_directory_path, "result.txt"), "a") as root:
                write_batch_info(root, args)
        reporter = _Reporter(script, args, synthetic)
        _recover_many([(j, f) for j in jobs for f in j.files], args, batch_size, on_window=reporter.flush if writer else None)
        if writer:
            reporter.flush()
            if traverse:
                with open(os.path.join(args.images_directory_path, "result.txt"), "a") as root:
                    root.write("=" * 40 + "Batch End" + "=" * 40 + "\n\n")


def process_single_directory(dir_path, args, *, batch_size=None):
    """One directory (extract.py:134-163)."""
    from . import dist as gdist
    batch_size = int(batch_size or getattr(args, "batch_size", 0) or 16)
    job = _DirJob(dir_path)
    if job.files:
        synthetic = _no_checkpoint(args.model_id)
        with _strictness(args, synthetic):
            load_models(args.model_id, allow_synthetic=_synthetic_allowed(args))
            _recover_many([(job, f) for f in job.files], args, batch_size)
        if gdist.rank_world()[0] == 0:
            _report(job, args, synthetic)


def build_parser():
    """extract.py:180-195: same flags and defaults."""
    import argparse

    class Parser(argparse.ArgumentParser):
        def parse_args(self, args=None, namespace=None):
            a = super().parse_args(args, namespace)
            if a.robust_soft:
                for flag, on in (("--soft 1", a.soft), ("--robust 1", a.robust), ("--window_soft", a.window_soft), ("--align", a.align != "none")):
                    if on:
                        self.error(f"--robust_soft cannot be combined with {flag}: it weights by levels AND tiles, in a decoder of its own")
            if a.soft and a.robust:
                self.error("--soft 1 cannot be combined with --robust 1: level weights and tile weights are separate votes")
            if a.soft and a.l != 1:
                self.error(f"--soft 1 cannot be combined with --l {a.l}: reliability levels are defined for one cipher bit per element (--l 1)")
            if a.window_soft and (a.soft or a.robust or a.align != "none"):
                self.error("--window_soft cannot be combined with --soft 1, --robust 1 or --align: it is a vote of its own")
            if a.window_soft and a.l == 1:
                self.error("--window_soft needs --l 2 or --l 4: at --l 1 the level-weighted vote is --soft 1")
            if a.align != "none" and (a.soft or a.robust or a.tamper_map):
                self.error("--align cannot be combined with --soft 1, --robust 1 or --tamper_map: the alignment search reads the reference's vote")
            if a.align_shift < 0 or (a.align == "none" and a.align_shift):
                self.error("--align_shift is a non-negative number of lattice steps and needs --align flips or --align d4")
            if a.ecc is not None or a.ecc_list > 1:
                try:
                    _ecc_wanted(a)
                except ValueError as e:
                    self.error(str(e))
            if a.original_payload_hex is not None:
                if a.ecc is None or a.original_message_hex is not None:
                    self.error("--original_payload_hex needs --ecc conv and takes the place of --original_message_hex: give one of the two")
                from . import ecc as E
                try:
                    a.original_message_hex = E.encode(bytes.fromhex(a.original_payload_hex), int(a.message_length), a.ecc).hex()
                except ValueError as e:
                    self.error(f"--original_payload_hex: {e}")
            if a.original_message_hex is None:
                self.error("the following arguments are required: --original_message_hex")
            return a

    parser = Parser(description="Extract watermark from a image")
    parser.add_argument("--model_id", default="stabilityai/stable-diffusion-2-1-base")
    parser.add_argument("--images_directory_path", default="", help="The path of directory containing images to process")
    parser.add_argument("--single_image_path", default="")
    parser.add_argument("--key_hex", required=True, help="Hexadecimal key used for encryption")
    parser.add_argument("--nonce_hex", required=True, help="Hexadecimal nonce used for encryption, It will use the fixed part of the key if nonce is none")
    parser.add_argument("--original_message_hex", default=None, help="Hexadecimal representation of the original message for accuracy calculation (required; "
                                                                      "with --ecc conv it stays the CODED message, or give --original_payload_hex)")
    parser.add_argument("--num_inference_steps", default=30, type=int, help="Number of inference steps for the model")
    parser.add_argument("--scheduler", default="DDIM", help="Choose a scheduler between 'DPMs' and 'DDIM' to inverse the image")
    parser.add_argument("--is_traverse_subdirectories", default=0, help="Whether to traverse subdirectories recursively")
    parser.add_argument("--l", default=1, type=int, help="The size of slide windows for m: cipher bits per lattice element (1, 2 or 4)")
    parser.add_argument("--width", type=int, default=1024, help="Width of the input image")
    parser.add_argument("--height", type=int, default=1024, help="Height of the input image")
    parser.add_argument("--message_length", type=int, default=1024, help="Length of the message in bits")
    # not a reference flag: opt in to seeded synthetic weights when --model_id is not a local checkpoint directory (results meaningless)
    parser.add_argument("--allow_synthetic_weights", action="store_true", help="run without a checkpoint (pipeline tests / benchmarks only)")
    parser.add_argument("--batch_size", type=int, default=16, help="(not a reference flag) images per device batch of the directory harness")
    parser.add_argument("--gpus", type=int, default=1, help="(not a reference flag) shard the images of a directory run over this many GPUs of the node: "
                                                           "one process per GPU, started here unless a launcher (torch.distributed.run) already did")
    parser.add_argument("--preflight", action="store_true", help="(not a reference flag) only check the multi-GPU control plane: per rank device check, RCCL init, one "
                                                                 "broadcast + all_gather_into_tensor + all_reduce under a hard time limit; exit 0 / 3")
    parser.add_argument("--robust", type=int, choices=[0, 1], default=0,
                        help="(not a reference flag) 1: decode with the tile-weighted vote (tamper.extract_robust): tiles that do not agree with the decoded "
                             "message lose their say; 0: the reference's vote")
    parser.add_argument("--tamper_map", default=None, metavar="DIR",
                        help="(not a reference flag) write DIR/<image>.tamper.npy / .tamper.png: per tile, the bits that agree with --original_message_hex")
    parser.add_argument("--tile", type=int, default=8, choices=codec.TILES, help="(not a reference flag) tile edge of --robust / --tamper_map, in lattice elements")
    parser.add_argument("--soft", type=int, choices=[0, 1], default=0,
                        help="(not a reference flag) 1: decode with the soft-decision vote (soft.extract_soft): every lattice element votes with a "
                             "reliability level taken from its magnitude; 0: the reference's vote.  Not with --robust 1, --l 1 only")
    parser.add_argument("--window_soft", type=int, default=0, choices=range(0, 16), metavar="L",
                        help="(not a reference flag) with --l 2 or 4: decode with the soft-decision vote for multi-bit windows (soft.extract_soft_l), every "
                             "cipher bit of a lattice element votes with one of L (1..15) levels taken from its distance to the quantiser boundaries that "
                             "would flip it; 0: the reference's vote.  Not with --soft 1, --robust 1 or --align")
    parser.add_argument("--robust_soft", type=int, default=0, choices=range(0, 16), metavar="L",
                        help="(not a reference flag) decode with the robust decode with levels (tamper.extract_robust_soft): every cipher bit votes with one "
                             "of L (1..15) reliability levels times the weight of its tile, the tiles re-weighted by their agreement with the decoded message "
                             "--iters times, in one launch; --tile, --iters, --sign_rounds, at any --l; 0: the reference's vote.  Not with --soft 1, --robust 1, "
                             "--window_soft or --align")
    parser.add_argument("--iters", type=int, default=2, choices=range(0, 9), metavar="I", help="(not a reference flag) --robust_soft: re-weighting rounds after the first vote (0..8)")
    parser.add_argument("--sign_rounds", type=int, default=1, choices=[0, 1],
                        help="(not a reference flag) --robust_soft: 1 takes the first vote at unit levels (safe against a pasted region louder than the image), "
                             "0 lets the levels count from the start (stronger where the damage is quiet)")
    parser.add_argument("--soft_levels", type=int, default=15, choices=range(1, 16), metavar="LEVELS", help="(not a reference flag) reliability levels of --soft 1 (1..15)")
    parser.add_argument("--soft_clip", type=float, default=2.5,
                        help="(not a reference flag) --soft 1: the top level starts at this many times the image's RMS")
    parser.add_argument("--strict_kernels", type=int, choices=[0, 1], default=None,
                        help="(not a reference flag) 1: raise when a GPU half-precision call would leave the hand-written kernels instead of warning "
                             "(default: 1; 0 opts into the library kernels, counted and warned about once per reason)")
    parser.add_argument("--align", default="none", choices=("none", "flips", "d4"),
                        help="(not a reference flag) read the message under the best alignment of the lattice (align.extract_aligned): flips = half turn and "
                             "the two mirrors, d4 = all eight orientations; none: the reference's vote as it is")
    parser.add_argument("--align_shift", type=int, default=0, metavar="R", help="(not a reference flag) with --align: also every lattice shift in [-R, R]^2")
    parser.add_argument("--ecc", default=None, choices=("conv", "conv23", "conv34"),
                        help="(not a reference flag) the message is an error-corrected payload (issue --ecc conv): the votes of whichever decoder is chosen "
                             "(plain, --soft 1, --window_soft L, --robust 1, --robust_soft L) are decoded by one Viterbi launch per batch, and after the "
                             "existing line comes 'payload <hex> crc ok|FAILED, corrected <flips> of <M>'.  Not with --align, --align_shift or --gpus above 1 yet")
    parser.add_argument("--ecc_list", type=int, default=1, choices=(1, 2, 4, 8),
                        help="(not a reference flag) with --ecc conv: the list read -- the decoder keeps this many best paths and the CRC picks among them; "
                             "the payload line gains ', list rank <r> of <L>[, <n> candidates pass]'.  1 (default): the plain read and today's text")
    parser.add_argument("--original_payload_hex", default=None,
                        help="(not a reference flag) with --ecc conv, in the place of --original_message_hex: the payload, encoded to the coded message first")
    return parser


def _init_ranks(args):
    """Join the process group a launcher prepared (RANK / WORLD_SIZE in the environment): RCCL with one GPU per rank, or gloo on a host
    without GPUs (CPU tests of the sharding logic)."""
    import torch.distributed as dist
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", "1"), ("RANK", "0"), ("LOCAL_RANK", "0")))
    if world != int(args.gpus):
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    backend = os.environ.get("GSW_DIST_BACKEND", "nccl" if torch.cuda.is_available() else "gloo")
    if backend == "nccl":
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        dist.init_process_group(backend)


def main(argv=None):
    """extract.py:179-211 (+ `--gpus N`: one process per GPU, the images of a directory run sharded over them)."""
    argv = list(sys.argv[1:] if argv is None else argv)
    args = build_parser().parse_args(argv)
    from . import launch
    if int(args.gpus) > 1 and not launch.under_launcher():
        # start the ranks BEFORE anything touches the GPU; plain children (never a re-exec), stopped by PID if one of them fails
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = {"PYTHONPATH": os.pathsep.join([root] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p])}
        raise SystemExit(launch.spawn_ranks([sys.executable, "-m", "gswm_amd.extract"] + argv, int(args.gpus), env_extra=env))
    if args.preflight:
        from . import dist as gdist
        if "WORLD_SIZE" not in os.environ:
            os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("MASTER_PORT") or str(launch._free_port()))
        backend = os.environ.get("GSW_DIST_BACKEND", "nccl" if torch.cuda.is_available() else "gloo")
        raise SystemExit(gdist.preflight_main(backend, float(os.environ.get("GSW_PREFLIGHT_TIMEOUT_S", "120"))))
    args.key = bytes.fromhex(args.key_hex)
    if args.nonce_hex != "":
        args.nonce = bytes.fromhex(args.nonce_hex)
    else:
        args.nonce = bytes.fromhex(args.key_hex[16:48])
    ranks = int(args.gpus) > 1
    if ranks:
        _init_ranks(args)
    try:
        if args.images_directory_path != "":
            process_directory(args)
        elif args.single_image_path != "":
            from . import dist as gdist
            if gdist.rank_world()[0] == 0:            # one image: nothing to shard
                with _strictness(args, _no_checkpoint(args.model_id)):
                    get_result_for_one_image(args)
        else:
            print("Please set the argument 'images_directory_path' or 'single_image_path'")
    finally:
        if ranks:
            import torch.distributed as dist
            if dist.is_initialized():
                dist.destroy_process_group()


if __name__ == "__main__":
    main()
