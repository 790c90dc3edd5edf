"""Restatement of softmax(q k^T * scale) v for the probes of the flash-attention kernel (csrc/gswm_attn.hip), in plain torch: operands whose answer is known to
the bit, the fp64 softmax they are checked with, and the rounding model of the kernel.  Shares no code with the device path; a plain module, no pytest plugin.

THE ONE-HOT PROBE.  A head has `d` columns; n + 2 of them are used (`columns`), the rest is zero.  With n = ceil(log2 Sk):
    key j (< Sk_valid)   its n index bits as +-A, then -n A in the bias column, then -(T_last - j // 64) in the ramp column (T_last: the last tile with a valid key)
    query i              the n bits of its target pi(i) as +-Bq, then Bq in the bias column, then rho(i) >= 0 in the ramp column
    score(i, j)        = -2 A Bq hamming(j, pi(i)) - rho(i) (T_last - j // 64)
an integer, a sum of integers, below 2^24: exact in fp32 in any summation order.  The target's score is exactly 0 when rho = 0 or the target lies in the last tile
(the only cases the schedules produce); every other valid key is at most -2 A Bq = -2048 raw, which at the default scale d^-1/2 is at least 233 in the base-2
exponent (head_dim 160: 2048 * log2(e) / sqrt(160)), so its probability is exactly 0 in fp32, the target's is exactly 1, the row sum is 1 and the output IS the
row V[b, pi(i), h d : (h + 1) d], bit for bit, in fp16 and in bf16.  V is random: any other key shows.  32, n * 32 <= 448 and tile distances <= 255 are exact in both
types, and so are the ramp weights 2048 (n_hi + 1) with n_hi <= 8 tile bits.
    Decoys.  Scores fall with the Hamming distance, so tiles in front of the target leave a running maximum and accumulators full of other keys' V rows, which the
target's tile has to wipe (alpha = 0).  The ramp makes that happen on EVERY tile: with rho = 2048 (n_hi + 1) the best key of tile t + 1 beats the best of tile t by at
least 2048 whatever their Hamming distances, so a query whose target lies in the last tile rescales at every tile ("last"); a target in the first tile and rho = 0
settle the maximum at once, and the kernel's skip branch runs ("first"); "mixed" has both kinds inside every wave, in every 16-lane row and in both halves.
    Padded keys j in [Sk_valid, Sk) score +2048 for every query (zero code, +64 in the bias column) and carry V rows of 1000: a leak changes bits.
    Two-hot.  Key j2 is given the code of key j1 (another tile; for the key-split form another split): both score 0, the weights are exactly 1/2 and the expected
row is round_T((v1 + v2) / 2): the fp32 sum of two T values is either exact or off by less than a quarter of a T ulp, so one rounding to T decides.

THE TOLERANCE CASES (rescales that are neither 0 nor 1 cannot be exact): `rescale_operands`, `dominant_operands`, `offset_operands`, compared with `softmax_fp64` of
the same rounded inputs within 5 u max|v| (u = 2^-11 fp16, 2^-8 bf16); `rounded_model` is the kernel's arithmetic model -- fp64 probabilities relative to the
row maximum, rounded to T, used for both the product and the row sum, the quotient rounded to T."""
import math

import torch

A = 32            # |key code entry|
BQ = 32           # |query code entry|
GAP = 2 * A * BQ   # raw score distance between Hamming neighbours
PAD_V = 1000.0
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def code_bits(Sk: int) -> int:
    return max(1, (Sk - 1).bit_length())


def columns(d: int, n: int) -> list:
    """the head columns of the n code entries, the bias and the ramp: spread over the head so that every 16-column k-slice of the first product carries some"""
    assert n + 2 <= d and math.gcd(7, d) == 1
    return [(7 * c + 3) % d for c in range(n + 2)]


def ramp_weight(Sk: int) -> int:
    return GAP * (max(0, code_bits(Sk) - 6) + 1)


def _bits(idx: torch.Tensor, n: int) -> torch.Tensor:
    """[..., n] of +-1.0: bit c of idx"""
    sh = torch.arange(n, device=idx.device)
    return (((idx.unsqueeze(-1) >> sh) & 1) * 2 - 1).to(torch.float32)


def probe_keys(B, H, d, Sk, Sk_valid, dtype, device="cpu") -> torch.Tensor:
    """k [B, Sk, H d] of the one-hot probe (the same rows for every batch and head)"""
    n = code_bits(Sk)
    col = columns(d, n)
    j = torch.arange(Sk, device=device)
    row = torch.zeros(Sk, d, device=device)
    row[:, col[:n]] = A * _bits(j, n)
    row[:, col[n]] = float(-n * A)
    row[:, col[n + 1]] = -(((Sk_valid - 1) // 64) - (j // 64)).to(torch.float32)
    row[Sk_valid:] = 0.0
    row[Sk_valid:, col[n]] = float(GAP // BQ)
    return row.to(dtype).view(1, Sk, 1, d).expand(B, Sk, H, d).reshape(B, Sk, H * d).contiguous()


def probe_queries(targets: torch.Tensor, rho: torch.Tensor, d, Sk, dtype) -> torch.Tensor:
    """q [B, Sq, H d] from targets / rho [B, H, Sq]"""
    B, H, Sq = targets.shape
    n = code_bits(Sk)
    col = columns(d, n)
    q = torch.zeros(B, H, Sq, d, device=targets.device)
    q[..., col[:n]] = BQ * _bits(targets, n)
    q[..., col[n]] = float(BQ)
    q[..., col[n + 1]] = rho.to(torch.float32)
    return q.to(dtype).transpose(1, 2).reshape(B, Sq, H * d).contiguous()


def probe_values(B, H, d, Sk, Sk_valid, dtype, seed, device="cpu") -> torch.Tensor:
    """v [B, Sk, H d]: N(0, 1) rounded to T and never zero (the sign of a zero that meets the +-0 products of the other keys depends on the order of the
    additions; every other value does not), rows of padded keys 1000"""
    v = _randn((B, Sk, H * d), seed, dtype, device)
    v[v == 0] = 1.0
    v[:, Sk_valid:] = PAD_V
    return v


def _coprime_from(s: int, m: int) -> int:
    while math.gcd(s, m) != 1:
        s += 1
    return s


def stride_of(Sk_valid: int) -> int:
    """the "stride" schedule's step: one tile and one slot, or the next number coprime to Sk_valid"""
    return _coprime_from(65, Sk_valid)


SCHEDULES = ("stride", "last", "first", "mixed")


def launch_cap(Sq: int, Sk_valid: int) -> int:
    return -(-Sk_valid // Sq) + 1


def launches(kind: str, Sq: int, Sk_valid: int) -> int:
    """launches after which the schedule has made every key of its range some query's target (per batch and head): the whole of [0, Sk_valid) for "stride", the
    last tile with a valid key for "last", the first tile for "first"; "mixed" is there for the two kinds of query side by side, not for coverage: one launch"""
    lo = 64 * ((Sk_valid - 1) // 64)
    return {"stride": -(-Sk_valid // Sq), "last": -(-(Sk_valid - lo) // Sq), "first": -(-min(64, Sk_valid) // Sq), "mixed": 1}[kind]


def schedule(kind: str, launch: int, B, H, Sq, Sk, Sk_valid, device="cpu"):
    """-> targets [B, H, Sq] (int64, in [0, Sk_valid)), rho [B, H, Sq] (the queries' ramp weights)"""
    i = torch.arange(Sq, device=device).view(1, 1, Sq)
    bh = (torch.arange(B, device=device).view(B, 1, 1) * H + torch.arange(H, device=device).view(1, H, 1))
    lo = 64 * ((Sk_valid - 1) // 64)                       # the last tile with a valid key: [lo, Sk_valid)
    n_last, n_first = Sk_valid - lo, min(64, Sk_valid)

    def walk(j, size):          # a bijection of [0, size) applied to the running query number j, shifted per batch and head
        return (_coprime_from(5, size) * j + bh) % size

    if kind == "stride":
        j = i + launch * Sq
        return ((stride_of(Sk_valid) * j + 17 * bh) % Sk_valid).expand(B, H, Sq).contiguous(), torch.zeros(B, H, Sq, device=device)
    w = float(ramp_weight(Sk))
    if kind == "last":
        return (lo + walk(i + launch * Sq, n_last)).expand(B, H, Sq).contiguous(), torch.full((B, H, Sq), w, device=device)
    if kind == "first":
        return walk(i + launch * Sq, n_first).expand(B, H, Sq).contiguous(), torch.zeros(B, H, Sq, device=device)
    if kind == "mixed":          # which kind a query is follows the parity of its number's bit count: no period, so no lane group of the kernel sees one kind only
        x = i + launch
        last = torch.zeros_like(x, dtype=torch.bool)
        for c in range(32):
            last = last ^ (((x >> c) & 1) == 1)
        t = torch.where(last, lo + walk(i + launch * Sq, n_last), walk(i + launch * Sq, n_first))
        return t.expand(B, H, Sq).contiguous(), (last * w).to(torch.float32).expand(B, H, Sq).contiguous()
    raise ValueError(kind)


def gather_rows(v: torch.Tensor, targets: torch.Tensor, H: int) -> torch.Tensor:
    """[B, Sq, H d]: row targets[b, h, i] of head h of v [B, Sk, H d]"""
    B, Sk, inner = v.shape
    d = inner // H
    bI = torch.arange(B, device=v.device).view(B, 1, 1)
    hI = torch.arange(H, device=v.device).view(1, 1, H)
    return v.view(B, Sk, H, d)[bI, targets.permute(0, 2, 1), hI].reshape(B, targets.shape[2], inner)


def two_hot_pairs(Sk: int, Sk_valid: int, launch: int, count: int = 16):
    """-> (j1 [M], j2 [M]): disjoint key pairs, j1 in the first quarter of the valid key tiles and j2 in the last (tile 0 and the last tile below four tiles), at
    slots that move through the tile; needs two tiles with a valid key"""
    nt = (Sk_valid + 63) // 64
    assert nt >= 2
    qt = max(1, nt // 4)
    j1, j2 = [], []
    for m in range(count):
        a = 64 * ((m + launch) % qt) + (37 * m + 5 + 11 * launch) % 64
        t2 = nt - 1 - (3 * m + launch) % qt
        width = min(64, Sk_valid - 64 * t2)
        b = 64 * t2 + (29 * m + 11 + 7 * launch) % width
        if a not in j1 and b not in j2:
            j1.append(a)
            j2.append(b)
    return torch.tensor(j1), torch.tensor(j2)


def two_hot(k: torch.Tensor, v: torch.Tensor, H: int, Sq: int, j1: torch.Tensor, j2: torch.Tensor):
    """-> (k', targets [B, H, Sq], expected [B, Sq, H d]): key j2[m] takes the code of key j1[m]; query i of (b, h) aims at pair (i + b H + h) % M"""
    B = k.shape[0]
    dev = k.device
    j1, j2 = j1.to(dev), j2.to(dev)
    k2 = k.clone()
    k2[:, j2] = k[:, j1]
    bh = (torch.arange(B, device=dev).view(B, 1, 1) * H + torch.arange(H, device=dev).view(1, H, 1))
    m = (torch.arange(Sq, device=dev).view(1, 1, Sq) + bh) % j1.numel()
    v64 = v.to(torch.float64)
    exp = ((gather_rows(v64, j1[m], H) + gather_rows(v64, j2[m], H)) * 0.5).to(v.dtype)
    return k2, j1[m], exp


# ---- fp64 evaluation
def heads(t: torch.Tensor, H: int) -> torch.Tensor:
    """[B, S, H d] -> [B, H, S, d] in fp64"""
    B, S, inner = t.shape
    return t.to(torch.float64).view(B, S, H, inner // H).transpose(1, 2)


def scores_fp64(q, k, H, scale, Sk_valid=None) -> torch.Tensor:
    """scaled scores [B, H, Sq, Sk] in fp64, padded keys at -inf"""
    s = heads(q, H) @ heads(k, H).transpose(-1, -2) * scale
    if Sk_valid is not None and Sk_valid < k.shape[1]:
        s[..., Sk_valid:] = -math.inf
    return s


def softmax_fp64(q, k, v, H, scale, Sk_valid=None) -> torch.Tensor:
    """[B, Sq, H d] in fp64: the plain reference"""
    p = torch.softmax(scores_fp64(q, k, H, scale, Sk_valid), dim=-1)
    o = p @ heads(v, H)
    return o.transpose(1, 2).reshape(q.shape[0], q.shape[1], -1)


def rounded_model(q, k, v, H, scale, Sk_valid=None) -> torch.Tensor:
    """[B, Sq, H d] of v's type: probabilities relative to the row maximum in fp64, ROUNDED to T; the convex sum of V rows with those weights (the same rounded
    numbers in the numerator and in the row sum); the quotient rounded to T"""
    s = scores_fp64(q, k, H, scale, Sk_valid)
    p = torch.exp(s - s.max(dim=-1, keepdim=True).values).to(v.dtype).to(torch.float64)
    o = (p @ heads(v, H)) / p.sum(dim=-1, keepdim=True)
    return o.transpose(1, 2).reshape(q.shape[0], q.shape[1], -1).to(v.dtype)


# ---- the tolerance cases: q, k, v [B, S, H d] of type T
def _randn(shape, seed, dtype, device, mul=1.0):
    """N(0, mul^2) rounded to T, drawn on the device it is for (the stream of a seed differs between devices; nothing here compares across them)"""
    g = torch.Generator(device=device).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=device) * mul).to(dtype)


def rescale_operands(B, H, d, Sq, Sk, dtype, seed, device="cpu"):
    """The per-tile maximum rises by about 3 nats per tile for the even queries and falls by as much for the odd ones (both kinds in every wave): key j carries its
    tile number in column 0, query i +-3 / scale there; the other columns are noise of about half a nat."""
    scale = d ** -0.5
    q = _randn((B, Sq, H, d), seed, dtype, device, 0.7 * d ** 0.25)
    k = _randn((B, Sk, H, d), seed + 1, dtype, device, 0.7 * d ** -0.25)
    v = _randn((B, Sk, H * d), seed + 2, dtype, device)
    q[..., 0] = torch.where(torch.arange(Sq, device=device) % 2 == 0, 3.0 / scale, -3.0 / scale).to(dtype).view(1, Sq, 1)
    k[..., 0] = (torch.arange(Sk, device=device) // 64).to(dtype).view(1, Sk, 1)
    return q.reshape(B, Sq, H * d), k.reshape(B, Sk, H * d), v


def dominant_operands(B, H, d, Sq, Sk, Sk_valid, dtype, seed, device="cpu"):
    """One key about 12 nats above Sk_valid - 1 equal ones (its index moves with batch and head): the tail's probabilities, e^-12 = 6e-6 each, are subnormal in fp16."""
    scale = d ** -0.5
    q = torch.zeros(B, Sq, H, d)
    k = torch.zeros(B, Sk, H, d)
    q[..., 1] = 32.0
    k[..., 1] = 1.0
    delta = round(12.0 / (32.0 * scale) * 8) / 8
    for b in range(B):
        for h in range(H):
            k[b, (977 * (b * H + h) + 61) % Sk_valid, h, 1] = 1.0 + delta
    v = _randn((B, Sk, H * d), seed, dtype, device)
    return q.reshape(B, Sq, H * d).to(dtype).to(device), k.reshape(B, Sk, H * d).to(dtype).to(device), v


def offset_operands(B, H, d, Sq, Sk, dtype, seed, device="cpu"):
    """Random scores of a few nats with +2000 raw added to every one (40 * 50 in column 2): the running maximum is large, the differences are not."""
    q = _randn((B, Sq, H, d), seed, dtype, device, 1.5)
    k = _randn((B, Sk, H, d), seed + 1, dtype, device)
    v = _randn((B, Sk, H * d), seed + 2, dtype, device)
    q[..., 2] = 40.0
    k[..., 2] = 50.0
    return q.reshape(B, Sq, H * d), k.reshape(B, Sk, H * d), v
