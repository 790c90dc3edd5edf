"""GPU: key-position probes of the flash-attention kernel (csrc/gswm_attn.hip), one case per `cover/` row of tests/golden/attn_plan_cases.tsv -- the table
tests/test_attn_plan_host.py proves against attn_decide, so every case is known to run the kernel form its tag names -- through the C ABI (gsw_attention_ws).

The operands come from tests/attention_reference.py (their claims are proven in fp64 by tests/test_attention_probe_host.py): softmax(q k^T scale) v is exactly ONE
row of a random V (or the mean of two), so the output is compared with torch.equal -- a lost, doubled or swapped key, a stale stage, a key range off by a tile, a
padded key that leaks, an accumulator the rescale forgets all change bits.  Rescales that are neither 0 nor 1 cannot be exact; three operand families drive them
and are held to 5 u max|v| against the fp64 softmax of the same rounded inputs (u = 2^-11 fp16, 2^-8 bf16: 2 u from rounding the probabilities that both the second
product and the row sum consume, u from the output, under 1 u from subnormal probabilities, the rest slack for fp32 accumulation and v_exp_f32).  Outputs live in
pattern-filled, guard-banded buffers (tests/poison.py)."""
import pytest
import torch

import attention_reference as R
import poison
from test_attention_probe_host import COVER, DTYPES, shape_of, valid_counts
from test_attn_plan_host import form_of

pytestmark = pytest.mark.gpu
IDS = [r["tag"][len("cover/"):] for r in COVER]
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    import gswm_amd  # noqa: F401
    from gswm_amd import _native
    return _native


_WS = {}
_V = {}


def launch(N, r, q, ldq, k, ldk, vt, out, ldo, Sk_valid, dtype):
    """gsw_attention_ws on the row's shape with the workspace the row records; q / k are device pointers or tensors"""
    B, H = int(r["B"]), int(r["H"])
    d, Sq0, Sk, _ = shape_of(r)
    nb = int(r["ws_bytes"])
    if nb and nb not in _WS:
        _WS[nb] = torch.empty(nb, dtype=torch.uint8, device=DEV)
    ptr = lambda t: t if isinstance(t, int) else t.data_ptr()
    rc = N.lib().gsw_attention_ws(ptr(q), ptr(k), vt.data_ptr(), ptr(out), B, H, d, Sq0, Sk, Sk_valid, ldq, ldk, ldo, float(d ** -0.5),
                                  N.GSW_F16 if dtype == torch.float16 else N.GSW_BF16, _WS[nb].data_ptr() if nb else None, nb, None)
    assert rc == 0, (r["tag"], rc)


def first_difference(got, want, H, targets=None):
    """(b, query, head, column), the two values and the query's target key at the first element whose bits differ"""
    ne = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
    if ne.numel() == 0:
        return None
    b, i, c = (int(x) for x in ne[0])
    d = got.shape[2] // H
    return {"differing": int(ne.shape[0]), "of": got.numel(), "b": b, "query": i, "head": c // d, "column": c % d, "got": float(got[b, i, c]), "want": float(want[b, i, c]),
            "target": None if targets is None else int(targets[b, c // d, i])}


class Case:
    """the operands of one row at one number of valid keys: keys and values once, an output inside guard bands"""

    def __init__(self, r, dtype, Sk_valid=None, seed=1):
        self.r, self.dtype = r, dtype
        self.B, self.H = int(r["B"]), int(r["H"])
        self.d, self.Sq, self.Sk, skv = shape_of(r)
        self.Skv = skv if Sk_valid is None else Sk_valid
        self.inner = self.H * self.d
        self.k = R.probe_keys(self.B, self.H, self.d, self.Sk, self.Skv, dtype, DEV)
        key = (r["tag"], dtype, seed)
        if key not in _V:          # (the random rows once per row of the table: the cases of a test differ in the padded rows only)
            _V.clear()
            _V[key] = R.probe_values(self.B, self.H, self.d, self.Sk, self.Sk, dtype, seed, DEV)
        self.v = _V[key].clone()
        self.v[:, self.Skv:] = R.PAD_V
        self.vt = self.v.transpose(1, 2).contiguous()
        self.ledger = poison.Ledger(poison.NAN)
        self.out = self.ledger.empty((self.B, self.Sq, self.inner), dtype, DEV)

    def wipe(self, t):
        t.view(torch.int16).fill_(poison._signed16(self.ledger.pattern))

    def one_hot(self, N, kind, ln, layouts=("rows",)):
        tg, rho = R.schedule(kind, ln, self.B, self.H, self.Sq, self.Sk, self.Skv, DEV)
        q = R.probe_queries(tg, rho, self.d, self.Sk, self.dtype)
        want = R.gather_rows(self.v, tg, self.H)
        inner = self.inner
        for layout in layouts:
            if layout == "rows":          # contiguous q and k
                self.wipe(self.out)
                launch(N, self.r, q, inner, self.k, inner, self.vt, self.out, inner, self.Skv, self.dtype)
                got = self.out
            elif layout == "slices":      # q and k as column slices of [B, S, 2 inner] rows, as the fused QK projection leaves them; the other half would dominate every score
                wq = torch.full((self.B, self.Sq, 2 * inner), 1000.0, dtype=self.dtype, device=DEV)
                wk = torch.full((self.B, self.Sk, 2 * inner), 1000.0, dtype=self.dtype, device=DEV)
                wq[:, :, :inner] = q
                wk[:, :, inner:] = self.k
                self.wipe(self.out)
                launch(N, self.r, wq, 2 * inner, wk.data_ptr() + 2 * inner, 2 * inner, self.vt, self.out, inner, self.Skv, self.dtype)
                got = self.out
            else:                         # ldo > inner: the columns between keep their pattern
                wide = self.ledger.empty((self.B, self.Sq, inner + 24), self.dtype, DEV)
                launch(N, self.r, q, inner, self.k, inner, self.vt, wide, inner + 24, self.Skv, self.dtype)
                got = wide[:, :, :inner]
                left = self.ledger.untouched(wide[:, :, inner:])
                assert left == self.B * self.Sq * 24, (self.r["tag"], kind, ln, "columns past the heads were written", self.ledger.where(wide[:, :, inner:], untouched=False))
            if not torch.equal(got.view(torch.int16), want.view(torch.int16)):
                raise AssertionError((self.r["tag"], str(self.dtype), "valid keys", self.Skv, kind, "launch", ln, layout, first_difference(got, want, self.H, tg)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("r", COVER, ids=IDS)
def test_one_hot_probe_every_key_every_schedule(lib, r, dtype):
    """Every key of the row is some query's target (per batch and head) over the launches of the "stride" schedule; "last" rescales at every tile, "first" at none,
    "mixed" both in one wave.  Contiguous rows, column slices, and once an output whose row stride is wider than the heads."""
    c = Case(r, dtype)
    for kind in R.SCHEDULES:
        L = R.launches(kind, c.Sq, c.Skv)
        assert L <= R.launch_cap(c.Sq, c.Skv)
        for ln in range(L):
            c.one_hot(lib, kind, ln, ("rows", "slices", "wide") if ln == 0 else ("rows", "slices"))
    c.ledger.check()          # (ragged rows: a store past Sq lands in a band)


PADDED = [r for r in COVER if form_of(r) != "ksplit"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("r", PADDED, ids=[r["tag"][len("cover/"):] for r in PADDED])
def test_one_hot_probe_with_padded_keys(lib, r, dtype):
    """Keys in [Sk_valid, Sk) score +2048 for every query and carry V rows of 1000: with 1 valid key, a tile boundary and its neighbours at both ends, Sk - 1,
    77 (of 128), and with the last two / four tiles -- a whole round of the four-stage loops -- masked."""
    d, Sq, Sk, _ = shape_of(r)
    counts = set(valid_counts(r))
    if form_of(r) == "dma" and Sk > 256:
        counts |= {Sk - 256, Sk - 255}
    for Skv in sorted(counts - {Sk}):
        c = Case(r, dtype, Skv, seed=2)
        for kind, ln in (("stride", 0), ("stride", 1), ("last", 0), ("mixed", 0)):
            c.one_hot(lib, kind, ln)
        c.ledger.check()


TWO_HOT = [r for r in COVER if int(r["Sk_valid"]) > 64]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("r", TWO_HOT, ids=[r["tag"][len("cover/"):] for r in TWO_HOT])
def test_two_hot_probe(lib, r, dtype):
    """Two keys in different tiles (different splits of the key-split form) share the code: weights exactly 1/2, the row is round_T((v1 + v2) / 2)."""
    c = Case(r, dtype, seed=3)
    for ln in range(3):
        j1, j2 = R.two_hot_pairs(c.Sk, c.Skv, ln)
        k2, tg, want = R.two_hot(c.k, c.v, c.H, c.Sq, j1, j2)
        q = R.probe_queries(tg, torch.zeros(c.B, c.H, c.Sq, device=DEV), c.d, c.Sk, dtype)
        c.wipe(c.out)
        launch(lib, r, q, c.inner, k2, c.inner, c.vt, c.out, c.inner, c.Skv, dtype)
        if not torch.equal(c.out.view(torch.int16), want.view(torch.int16)):
            raise AssertionError((r["tag"], str(dtype), "launch", ln, "pairs", list(zip(j1.tolist(), j2.tolist())), first_difference(c.out, want, c.H, tg)))
    c.ledger.check()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("r", COVER, ids=IDS)
def test_rescales_that_are_not_exact_stay_within_5u(lib, r, dtype):
    """Per-tile maxima that rise by about 3 nats per tile for the even queries and fall for the odd ones; one key 12 nats above a flat tail (subnormal fp16
    probabilities); +2000 raw on every score.  Against the fp64 softmax of the same rounded inputs (three images of the batch at most), |got - ref| <= 5 u max|v|
    per image and head.  Measured on an MI355X over all rows, in units of u max|v| (printed per case): rescale <= 0.40, dominant <= 0.58, offset <= 0.69 in fp16;
    0.40, 0.47, 0.68 in bf16.  (The bound stays the derived one: a kernel that, say, takes another query block's row sum measures hundreds.)"""
    B, H = int(r["B"]), int(r["H"])
    d, Sq, Sk, Skv = shape_of(r)
    u = R.U[dtype]
    inner = H * d
    ledger = poison.Ledger(poison.NAN)
    measured = {}
    for name, (q, k, v) in (("rescale", R.rescale_operands(B, H, d, Sq, Sk, dtype, 21, DEV)), ("dominant", R.dominant_operands(B, H, d, Sq, Sk, Skv, dtype, 22, DEV)),
                            ("offset", R.offset_operands(B, H, d, Sq, Sk, dtype, 23, DEV))):
        out = ledger.empty((B, Sq, inner), dtype, DEV)
        launch(lib, r, q, inner, k, inner, v.transpose(1, 2).contiguous(), out, inner, Skv, dtype)
        assert ledger.untouched(out) == 0
        bs = sorted({0, B // 2, B - 1})
        ref = R.softmax_fp64(q[bs], k[bs], v[bs], H, d ** -0.5, Skv)
        vmax = v[bs, :Skv].double().abs().view(len(bs), Skv, H, d).amax(dim=(1, 3))                      # per image and head: the rows a query of that head can mix
        err = (out[bs].double() - ref).abs().view(len(bs), Sq, H, d).amax(dim=(1, 3))
        measured[name] = round((err / (u * vmax)).max().item(), 3)
    ledger.check()
    print(f"\n{r['tag']} {dtype}: max|got - ref| / (u max|v|) = {measured}")
    assert all(e <= 5.0 for e in measured.values()), measured
