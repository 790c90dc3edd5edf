"""GPU: the kernels on poisoned, guard-banded buffers (tests/poison.py).  Every case takes edge shapes the existing parity tests already use, runs the operation
through its Python wrapper three times -- plainly, under poisoned(Ledger(NAN)) and under poisoned(Ledger(FINITE)), inputs wrapped, split-K / key-split scratch
from the ledger -- and asserts
  (a) every guard band still holds the pattern (no store outside a buffer),
  (b) no output element the kernel's contract says it writes still holds the pattern, and the regions it is documented NOT to write (PF guard rows, the
      border behind gn_only=True, columns past N of a strided output, the other half of a shared `out`) are untouched,
  (c) the three results are the same bits (nothing depends on memory the kernel should not read; the FINITE run is there because max-reductions swallow NaN),
  (d) the result meets the reference and tolerance of the kernel's own test file (cited at each case; no tolerance is new here).
One-byte outputs (images, packed bits, key stream) legitimately contain the pattern's bytes, so (b) cannot count them: an unwritten byte shows in (c), where the
two patterns differ in both byte positions, and in (d), which is equality for them."""
import contextlib
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

from conftest import README_KEY, README_NONCE  # noqa: E402
from poison import FINITE, NAN, Ledger, poisoned, scratch  # noqa: E402

pytestmark = pytest.mark.gpu
KEY, NONCE = bytes.fromhex(README_KEY), bytes.fromhex(README_NONCE)
F16, BF16 = torch.float16, torch.bfloat16


@pytest.fixture(scope="module")
def G():
    import gswm_amd  # noqa: F401
    from gswm_amd import _native, codec, imaging, pf, unet, vae, xattn
    return types.SimpleNamespace(pf=pf, unet=unet, vae=vae, codec=codec, imaging=imaging, xattn=xattn, N=_native, lib=_native.lib())


@contextlib.contextmanager
def setting(obj, **kw):
    """module switches for the block (the dispatch thresholds the other test modules pin in their fixtures)"""
    old = {k: getattr(obj, k) for k in kw}
    for k, v in kw.items():
        setattr(obj, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(obj, k, v)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the three runs
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
class Out:
    """What one run hands back.  written: name -> tensor the contract says is written in full (checked (b), compared (c)); kept: name -> view that must still be
    all pattern; same: name -> tensor that is only compared (in-place targets, whose previous contents were data, not pattern)."""

    def __init__(self, written=None, kept=None, same=None):
        self.written, self.kept, self.same = dict(written or {}), dict(kept or {}), dict(same or {})

    def add(self, other: "Out", prefix: str = ""):
        for mine, theirs in ((self.written, other.written), (self.kept, other.kept), (self.same, other.same)):
            mine.update({prefix + k: v for k, v in theirs.items()})
        return self

    def compared(self):
        return {**self.written, **self.same}


_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _bits(t):
    t = t.contiguous()
    return t.view(_INT[t.element_size()])


def _alloc(L, shape, dtype):
    """an output buffer a case hands to the C ABI itself (the wrappers' own come from poisoned())"""
    return torch.empty(shape, dtype=dtype, device="cuda") if L is None else L.empty(shape, dtype, "cuda")


def three_ways(G, case, inputs, ws_bytes=0):
    """case(inputs, ledger or None) -> Out.  Returns the clean run's Out for the caller's reference check (d)."""
    clean = case(dict(inputs), None)
    torch.cuda.synchronize()
    snaps = []
    for name, pattern in (("NAN", NAN), ("FINITE", FINITE)):
        L = Ledger(pattern)
        try:
            with poisoned(L):
                inp = {k: (L.wrap(v) if isinstance(v, torch.Tensor) and v.is_cuda else v) for k, v in inputs.items()}
                with (G.pf.splitk_workspace(scratch(L, ws_bytes)) if ws_bytes else contextlib.nullcontext()):
                    r = case(inp, L)
            torch.cuda.synchronize()
            L.check()                                                                                   # (a)
            for k, t in r.written.items():                                                              # (b)
                if t.element_size() > 1:
                    n = L.untouched(t)
                    assert n == 0, f"{k}: {n} of {t.numel()} elements were never written ({name} run) -- {L.where(t)}"
            for k, t in r.kept.items():
                n = L.untouched(t)
                assert n == t.numel(), f"{k}: {t.numel() - n} of {t.numel()} elements were written, the contract says none ({name} run) -- {L.where(t, untouched=False)}"
            assert set(r.compared()) == set(clean.compared())
            snaps.append({k: _bits(t).clone() for k, t in r.compared().items()})
        finally:
            L.release()
    for k, t in clean.compared().items():                                                               # (c)
        c = _bits(t)
        assert torch.equal(snaps[0][k], snaps[1][k]), f"{k}: the NAN and the FINITE run differ in {int((snaps[0][k] != snaps[1][k]).sum())} elements"
        assert torch.equal(c, snaps[0][k]), f"{k}: the poisoned runs differ from the clean run in {int((c != snaps[0][k]).sum())} elements"
    return clean


def _rel(y, ref):
    return (y.float() - ref.float()).abs().max().item() / max(ref.float().abs().max().item(), 1e-6)


def _borders(y):
    g = y.grid
    return {"border.top": g[:, 0], "border.bottom": g[:, -1], "border.left": g[:, :, 0], "border.right": g[:, :, -1]}


def pf_out(y, border=True) -> Out:
    """a PF tensor a kernel produced: interior written, border written (zeros) or -- behind gn_only=True -- left alone, guard rows never written (pf.PF.empty:
    'guard rows ... need to exist but not to hold anything in particular')"""
    o = Out(written={"interior": y.interior}, kept={"guard.front": y.buf[: y.G], "guard.back": y.buf[y.G + y.M:]})
    (o.written if border else o.kept).update(_borders(y))
    return o


def pf_in(pf, x):
    """NCHW -> PF the way the issue asks for inputs: PF.empty (pattern under poison: the guard rows stay pattern), a zeroed border, the interior copied"""
    B, C, H, W = x.shape
    p = pf.PF.empty(B, H, W, C, x.dtype, x.device)
    g = p.grid
    g[:, 0].zero_(); g[:, -1].zero_(); g[:, :, 0].zero_(); g[:, :, -1].zero_()
    p.interior.copy_(x.permute(0, 2, 3, 1))
    return p


def _zero_border(y):
    g = y.grid
    return bool(g[:, 0].abs().max() == 0 and g[:, -1].abs().max() == 0 and g[:, :, 0].abs().max() == 0 and g[:, :, -1].abs().max() == 0)


def _rnd(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g)


TOL = {F16: 2e-3, BF16: 1.6e-2}          # tests/test_gpu_gemm.py:_tol, tests/test_gpu_splitk.py:TOL


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# matmul engine (tests/test_gpu_gemm.py, test_gpu_splitk.py, test_gpu_lnfold.py, test_gpu_qkv.py, test_gpu_small.py)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def engine(G):
    """pf.gemm on the matmul ENGINE also at <= 128 rows (as the fixtures of test_gpu_gemm.py / test_gpu_splitk.py pin it)"""
    with setting(G.pf, SMALL_GEMM_MAX_ROWS=0):
        yield G.pf


_TOK = {1: (1, 1, 1), 8: (1, 2, 4), 513: (1, 27, 19), 777: (1, 21, 37), 1000: (2, 20, 25)}          # M token rows as (images, H, W)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("M", [1, 8, 513, 777, 1000])
def test_gemm_every_mode_ragged_rows(G, engine, dtype, M):
    """plain (+ residual), GEGLU, transposed and tokens -> PF (in-place residual) at ragged M; references and bounds of tests/test_gpu_gemm.py"""
    pf = engine
    K, N, I = 320, 320, 160
    r = _rnd(M)
    Mt = M // 8 * 8                                                          # transposed output: tokens % 8 == 0 (test_gpu_gemm.py:139)
    B, H, W = _TOK[M]
    inp = dict(x=r(M, K).to(dtype).cuda(), w=(r(N, K) * K ** -0.5).to(dtype).cuda(), b=r(N).to(dtype).cuda(), res=r(M, N).to(dtype).cuda(),
               wg=(r(2 * I, K) * K ** -0.5).to(dtype).cuda(), bg=(0.5 * r(2 * I)).to(dtype).cuda(), base=r(B, N, H, W).to(dtype).cuda())
    wp, bp = pf.pack_geglu_weight(inp["wg"], inp["bg"])
    inp.update(wp=wp, bp=bp)

    def case(i, L):
        o = Out(written={"plain": pf.gemm(i["x"], i["w"], i["b"]), "resid": pf.gemm(i["x"], i["w"], None, resid=i["res"]),
                         "geglu": pf.gemm(i["x"], i["wp"], i["bp"], mode="geglu")})
        if Mt:
            o.written["trans"] = pf.gemm(i["x"][:Mt].reshape(1, Mt, K), i["w"], i["b"], mode="trans", tokens=Mt)
        X = pf_in(pf, i["base"])
        pf.gemm(i["x"], i["w"], i["b"], resid=X.rows, mode="tok2pf", tokens=H * W, width=W, out=X.rows)
        o.same["tok2pf"] = X.rows
        o.kept.update({"tok2pf.guard.front": X.buf[: X.G], "tok2pf.guard.back": X.buf[X.G + X.M:]})          # test_gpu_gemm.py:101
        o.X = X
        return o

    c = three_ways(G, case, inp)
    x, w, b = inp["x"].float(), inp["w"].float(), inp["b"].float()
    ref = x @ w.T + b
    tol = TOL[dtype]
    assert _rel(c.written["plain"], ref) <= tol
    ref2 = x @ w.T + inp["res"].float()
    assert _rel(c.written["resid"], ref2) <= 2 * tol
    h = (x @ inp["wg"].float().T + inp["bg"].float()).to(dtype).float()
    refg = h[:, :I] * F.gelu(h[:, I:])
    assert (c.written["geglu"].float() - refg).abs().max().item() <= 2 * tol * max(1.0, refg.abs().max().item())
    if Mt:
        assert _rel(c.written["trans"][0], ref[:Mt].T) <= tol
    refp = ref.view(B, H, W, N).permute(0, 3, 1, 2) + inp["base"].float()
    assert _rel(c.X.to_nchw(), refp) <= 2 * tol and _zero_border(c.X)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("M,K,N", [(300, 128, 8), (777, 256, 136), (64, 64, 168), (256, 1280, 328)])
def test_gemm_partial_last_column_tile_and_strided_destination(G, engine, dtype, M, K, N):
    """N off the 160-column tile; gemm_strided into a column slice: nothing is written past column N (tests/test_gpu_gemm.py:122-141)"""
    pf = engine
    r = _rnd(M + N)
    inp = dict(x=r(M, K).to(dtype).cuda(), w=(r(N, K) * K ** -0.5).to(dtype).cuda(), b=r(N).to(dtype).cuda(), res=r(M, N).to(dtype).cuda())

    def case(i, L):
        wide = _alloc(L, (M, N + 24), dtype)
        if L is None:
            wide.fill_(7.0)
        pf.gemm_strided(i["x"], i["w"], wide[:, :N], i["b"])
        o = Out(written={"full": pf.gemm(i["x"], i["w"], i["b"], resid=i["res"]), "strided": wide[:, :N]})
        if L is not None:
            o.kept["strided.past_N"] = wide[:, N:]
        return o

    c = three_ways(G, case, inp)
    ref = inp["x"].float() @ inp["w"].float().T + inp["b"].float()
    tol = 4e-3 if dtype == F16 else 3e-2
    scale = max(1.0, (ref + inp["res"].float()).abs().max().item())
    assert (c.written["full"].float() - ref - inp["res"].float()).abs().max().item() <= tol * scale
    assert (c.written["strided"].float() - ref).abs().max().item() <= tol * scale


@pytest.mark.parametrize("k", [2, 7])
def test_split_k_on_ledger_scratch(G, engine, k):
    """forced k-way splits, the slabs in pattern-filled scratch: dense rows (ragged M and N), GEGLU, transposed, tokens -> PF, convolution with row bias and
    residual, the three-segment launch, the upsampler (tests/test_gpu_splitk.py, its shapes and bounds)"""
    pf, dtype = engine, F16
    r = _rnd(k)
    h = lambda *s, scale=1.0: (r(*s) * scale).to(dtype).cuda()
    dense = [(200, 5120, 1280), (256, 1280, 328), (1, 1280, 640)]
    inp = {}
    for j, (M, K, N) in enumerate(dense):
        inp.update({f"x{j}": h(M, K), f"w{j}": h(N, K, scale=K ** -0.5), f"b{j}": h(N), f"r{j}": h(M, N)})
    Kg, I = 1280, 640
    inp.update(xg=h(256, Kg), wg=h(2 * I, Kg, scale=Kg ** -0.5), bg=h(2 * I), xs=h(3, 64, 1280), tok=h(2, 64, 1280), base=h(2, 1280, 8, 8))
    wp, bp = pf.pack_geglu_weight(inp["wg"], inp["bg"])
    inp.update(wp=wp, bp=bp)
    # convolutions: (1, 128, 136, 10, 6) 3x3 and one image's 8 x 8 level at 1280 channels (test_gpu_splitk.py:CONVS), three segments, up2x
    inp.update(cx=h(1, 128, 10, 6), cw=h(136, 128, 3, 3, scale=(9 * 128) ** -0.5), cb=h(136), crb=h(1, 136), cres=h(1, 136, 10, 6),
               dx=h(1, 1280, 8, 8), dw=h(1280, 1280, 3, 3, scale=(9 * 1280) ** -0.5), db=h(1280), sx1=h(1, 1280, 8, 8), sx2=h(1, 640, 8, 8),
               sw1=h(1280, 1920, scale=1920 ** -0.5))
    inp.update(cwp=pf.pack_conv_weight(inp["cw"]), dwp=pf.pack_conv_weight(inp["dw"]), dwu=pf.pack_upsample_weight(inp["dw"]))
    inp["wcat"] = torch.cat([inp["dwp"], inp["sw1"]], dim=1).contiguous()

    def case(i, L):
        o = Out()
        pf.LAUNCH_LOG = log = []
        try:
            with setting(pf, SPLITK_MAX=k):
                for j in range(len(dense)):
                    o.written[f"dense{j}"] = pf.gemm(i[f"x{j}"], i[f"w{j}"], i[f"b{j}"])
                    o.written[f"dense{j}+res"] = pf.gemm(i[f"x{j}"], i[f"w{j}"], i[f"b{j}"], resid=i[f"r{j}"])
                o.written["geglu"] = pf.gemm(i["xg"], i["wp"], i["bp"], mode="geglu")
                o.written["trans"] = pf.gemm(i["xs"], i["w0"][:, :1280].contiguous(), i["b0"], mode="trans", tokens=64)
                X = pf_in(pf, i["base"])
                pf.gemm(i["tok"], i["w0"][:, :1280].contiguous(), i["b0"], resid=X.rows, mode="tok2pf", tokens=64, width=8, out=X.rows)
                o.same["tok2pf"] = X.rows
                o.X = X
                o.conv = pf.conv_pf(pf_in(pf, i["cx"]), i["cwp"], i["cb"], rowbias=i["crb"], resid=pf_in(pf, i["cres"]))
                o.deep = pf.conv_pf(pf_in(pf, i["dx"]), i["dwp"], i["db"])
                o.seg3 = pf.conv3x3_res_pf(pf_in(pf, i["dx"]), i["wcat"], i["db"], x1=pf_in(pf, i["sx1"]), x2=pf_in(pf, i["sx2"]))
                o.up = pf.conv_up2x_pf(pf_in(pf, i["dx"]), i["dwu"], i["db"])
        finally:
            pf.LAUNCH_LOG = None
        for nm in ("conv", "deep", "seg3", "up"):
            o.add(pf_out(getattr(o, nm)), nm + ".")
        o.splits = [e.splits for e in log]
        return o

    c = three_ways(G, case, inp, ws_bytes=G.pf.SPLITK_BYTES)
    assert max(c.splits) == k                                                 # the forced split count really ran
    for j in range(len(dense)):
        ref = inp[f"x{j}"].float() @ inp[f"w{j}"].float().T + inp[f"b{j}"].float()
        assert _rel(c.written[f"dense{j}"], ref) <= TOL[dtype] and _rel(c.written[f"dense{j}+res"], ref + inp[f"r{j}"].float()) <= 2 * TOL[dtype]
    proj = inp["xg"].float() @ inp["wg"].float().T + inp["bg"].float()
    assert _rel(c.written["geglu"], proj[:, :I] * F.gelu(proj[:, I:])) <= 3e-3
    w0, b0 = inp["w0"][:, :1280].float(), inp["b0"].float()
    assert _rel(c.written["trans"], (inp["xs"].float() @ w0.T + b0).transpose(1, 2)) <= 2e-3
    refP = inp["base"].float() + (inp["tok"].float() @ w0.T + b0).view(2, 8, 8, 1280).permute(0, 3, 1, 2)
    assert _rel(c.X.to_nchw(), refP) <= 4e-3 and _zero_border(c.X)
    refc = F.conv2d(inp["cx"].float(), inp["cw"].float(), inp["cb"].float(), padding=1) + inp["crb"].float()[:, :, None, None] + inp["cres"].float()
    assert _rel(c.conv.to_nchw(), refc) <= 2e-3 and _zero_border(c.conv)
    refd = F.conv2d(inp["dx"].float(), inp["dw"].float(), inp["db"].float(), padding=1)
    assert _rel(c.deep.to_nchw(), refd) <= 2e-3 and _zero_border(c.deep)
    ref3 = refd + F.conv2d(torch.cat([inp["sx1"], inp["sx2"]], 1).float(), inp["sw1"].float()[:, :, None, None])
    assert _rel(c.seg3.to_nchw(), ref3) <= 2e-3
    refu = F.conv2d(F.interpolate(inp["dx"].float(), scale_factor=2.0, mode="nearest"), inp["dw"].float(), inp["db"].float(), padding=1)
    assert _rel(c.up.to_nchw(), refu) <= 4e-3 and _zero_border(c.up)


@pytest.mark.parametrize("M,C,N", [(1024, 320, 640), (264, 328, 320)])
def test_gemm_ln_row_records_and_finish(G, engine, M, C, N):
    """the producer's row records, gsw_ln_rowstats_finish and the folded GEMM in its three modes (tests/test_gpu_lnfold.py: bounds 3e-3 / rtol 2e-4)"""
    pf = engine
    r = _rnd(M + C + N)
    h = lambda *s, scale=1.0, off=0.0: (r(*s) * scale + off).half().cuda()
    inp = dict(a=h(M, 320), w=h(C, 320, scale=320 ** -0.5), b=h(C, off=2.0), res=h(M, C), gamma=h(C, scale=0.3, off=1.0), beta=h(C, scale=0.2),
               w2=h(N, C, scale=C ** -0.5), b2=h(N))
    fold = pf.fold_ln_weights(inp["w2"], inp["b2"], inp["gamma"], inp["beta"])
    foldg = pf.fold_ln_weights(inp["w2"], inp["b2"], inp["gamma"], inp["beta"], geglu=True)
    inp.update(f0=fold[0], f1=fold[1], f2=fold[2], g0=foldg[0], g1=foldg[1], g2=foldg[2])
    ragged = C % 64 != 0                                                      # K of the folded GEMM must be a multiple of 64: (264, 328) is about the records

    def case(i, L):
        with setting(pf, FOLD_LN_MIN_ROWS=0):
            x = pf.gemm(i["a"], i["w"], i["b"], resid=i["res"], rowstats=True)
            rs = x._gsw_rowstats
            st = pf.ln_stat(x, 1e-5)
            o = Out(written={"x": x, "records": rs[0][: M * rs[1] * 2], "stat": st})
            if not ragged:
                o.written["plain"] = pf.gemm_ln(x, st, i["f0"], i["f1"], i["f2"])
                o.written["geglu"] = pf.gemm_ln(x, st, i["g0"], i["g1"], i["g2"], mode="geglu")
                o.written["trans"] = pf.gemm_ln(x.view(4, M // 4, C), st, i["f0"], i["f1"], i["f2"], mode="trans", tokens=M // 4)
        o.slots = rs[1]
        return o

    c = three_ways(G, case, inp)
    x = c.written["x"]
    xf = x.double()
    rec = c.written["records"].view(M, c.slots, 2).double()
    assert c.slots == 2 * ((C + 159) // 160)
    assert torch.allclose(rec[..., 0].sum(1), xf.sum(1), rtol=1e-5, atol=1e-2) and torch.allclose(rec[..., 1].sum(1), (xf * xf).sum(1), rtol=1e-5, atol=1e-2)
    rstd = (xf.var(1, unbiased=False) + 1e-5).rsqrt()
    st = c.written["stat"]
    assert torch.allclose(st[:, 0].double(), rstd, rtol=2e-4) and torch.allclose(st[:, 1].double(), -rstd * xf.mean(1), rtol=2e-4, atol=1e-4)
    if not ragged:
        proj = F.layer_norm(x.float(), (C,), inp["gamma"].float(), inp["beta"].float(), 1e-5) @ inp["w2"].float().T + inp["b2"].float()
        assert _rel(c.written["plain"], proj) <= 3e-3
        assert _rel(c.written["geglu"], proj[:, : N // 2] * F.gelu(proj[:, N // 2:])) <= 3e-3
        assert _rel(c.written["trans"], proj.view(4, M // 4, N).transpose(1, 2)) <= 3e-3


@pytest.mark.parametrize("B,S,K,inner,bias", [(1, 64, 1280, 1280, False), (2, 128, 320, 320, True), (3, 256, 1280, 1280, False)])
def test_gemm_qkv(G, engine, B, S, K, inner, bias):
    """tests/test_gpu_qkv.py: bound 2e-3 of the fp32 projection"""
    pf = engine
    r = _rnd(B + S + K)
    inp = dict(x=r(B, S, K).half().cuda(), w=(r(3 * inner, K) * K ** -0.5).half().cuda())
    if bias:
        inp["b"] = r(3 * inner).half().cuda()

    def case(i, L):
        qk, vt = pf.gemm_qkv(i["x"], i["w"], 2 * inner, i.get("b"))
        return Out(written={"qk": qk, "vt": vt})

    c = three_ways(G, case, inp)
    ref = inp["x"].float() @ inp["w"].float().T + (inp["b"].float() if bias else 0.0)
    assert (c.written["qk"].float() - ref[..., : 2 * inner]).abs().max().item() <= 2e-3 * ref.abs().max().item()
    assert (c.written["vt"].float() - ref[..., 2 * inner:].transpose(1, 2)).abs().max().item() <= 2e-3 * ref.abs().max().item()


@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
@pytest.mark.parametrize("M,K,N", [(64, 1280, 1280), (80, 128, 48), (16, 5120, 160)])
def test_gemm_small_every_configuration(G, cfg, M, K, N):
    """gsw_gemm_small through the C ABI as tests/test_gpu_small.py drives it: plain, residual + row records, transposed, GEGLU, tokens -> PF in place"""
    from test_gpu_small import _small
    dtype = F16
    r = _rnd(M + K + N + cfg)
    inp = dict(x=r(M, K).to(dtype).cuda(), w=(r(N, K) * K ** -0.5).to(dtype).cuda(), b=r(N).to(dtype).cuda(), res=r(M, N).to(dtype).cuda())
    geglu = N % 32 == 0                                                       # the kernel's GEGLU epilogue pairs 16-column blocks: 48 columns are refused
    if geglu:
        inp["wp"], inp["bp"] = G.pf.pack_geglu_weight(inp["w"], inp["b"])
    S = M // 2 if (M // 2) % 4 == 0 else M
    tokpf = N % 16 == 0 and M % 16 == 0
    if tokpf:
        inp["base"] = r(M // 16, N, 2, 8).to(dtype).cuda()

    def case(i, L):
        o = Out()
        y, y2, yt = _alloc(L, (M, N), dtype), _alloc(L, (M, N), dtype), _alloc(L, (M // S, N, S), dtype)
        rec = _alloc(L, (M * ((N + 31) // 32) * 2,), torch.float32)
        assert _small(G, i["x"], i["w"], i["b"], y, "plain", cfg)[0] == 0
        rc, slots = _small(G, i["x"], i["w"], None, y2, "plain", cfg, resid=i["res"], rowstats=rec)
        assert rc == 0 and slots > 0
        assert _small(G, i["x"], i["w"], i["b"], yt, "trans", cfg, S=S)[0] == 0
        o.written.update(plain=y, resid=y2, trans=yt, records=rec[: M * slots * 2])
        if L is not None:
            o.kept["records.tail"] = rec[M * slots * 2:]
        if geglu:
            yg = _alloc(L, (M, N // 2), dtype)
            assert _small(G, i["x"], i["wp"], i["bp"], yg, "geglu", cfg)[0] == 0
            o.written["geglu"] = yg
        if tokpf:
            X = pf_in(G.pf, i["base"])
            assert _small(G, i["x"], i["w"], i["b"], X.rows, "tok2pf", cfg, resid=X.rows, S=16, Wimg=8, ldr=N, ldy=N)[0] == 0
            o.same["tok2pf"] = X.rows
            o.kept.update({"tok2pf.guard.front": X.buf[: X.G], "tok2pf.guard.back": X.buf[X.G + X.M:]})
            o.X = X
        o.slots = slots
        return o

    c = three_ways(G, case, inp)
    tol = 2e-3
    x, w = inp["x"].float(), inp["w"].float()
    ref = x @ w.t() + inp["b"].float()
    assert _rel(c.written["plain"], ref) <= tol
    ref2 = (x @ w.t()).to(dtype).float() + inp["res"].float()
    assert _rel(c.written["resid"], ref2) <= tol
    assert (c.written["trans"].float() - ref.view(M // S, S, N).transpose(1, 2)).abs().max().item() <= tol * ref.abs().max().item()
    rsum = c.written["records"].view(M, c.slots, 2).double().sum(dim=1)
    y2 = c.written["resid"].double()
    assert torch.allclose(rsum[:, 0], y2.sum(dim=1), rtol=1e-4, atol=1e-2) and torch.allclose(rsum[:, 1], (y2 ** 2).sum(dim=1), rtol=1e-4, atol=1e-2)
    if geglu:
        refg = ref[:, : N // 2].to(dtype).float() * F.gelu(ref[:, N // 2:].to(dtype).float()).to(dtype).float()
        assert (c.written["geglu"].float() - refg).abs().max().item() <= 4e-3 * max(1.0, refg.abs().max().item())
    if tokpf:
        refp = ref.to(dtype).float().view(M // 16, 2, 8, N) + inp["base"].float().permute(0, 2, 3, 1)
        assert _rel(c.X.interior, refp) <= 2e-3 and _zero_border(c.X)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# convolutions (tests/test_gpu_pf.py, test_gpu_small.py, test_gpu_gn_colstats.py)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("B,C,N,H,W,ks,stride", [(3, 128, 64, 10, 6, 3, 1), (3, 128, 136, 5, 7, 3, 1), (2, 64, 128, 8, 16, 1, 1), (2, 64, 64, 8, 16, 3, 2),
                                                  (2, 128, 320, 10, 6, 3, 2), (3, 64, 160, 5, 7, 1, 1), (2, 128, 192, 8, 16, 3, 2)])
def test_conv_pf_small_lattices(G, dtype, B, C, N, H, W, ks, stride):
    """3x3 and 1x1, stride 1 and 2, on the 5 x 7, 10 x 6 and 8 x 16 lattices, with row bias and residual, and with no optional operand; both kernels (64 output
    columns: gsw_conv_gemm_kernel; from 128 up: the engine).  tests/test_gpu_pf.py:test_conv_pf_vs_torch_fp32"""
    pf = G.pf
    r = _rnd(C + N + H)
    Ho, Wo = H // stride, W // stride
    inp = dict(x=r(B, C, H, W).to(dtype).cuda(), w=(r(N, C, ks, ks) * (C * ks * ks) ** -0.5).to(dtype).cuda(), b=r(N).to(dtype).cuda(),
               rb=r(B, N).to(dtype).cuda(), res=r(B, N, Ho, Wo).to(dtype).cuda())
    inp["wp"] = pf.pack_conv_weight(inp["w"])

    def case(i, L):
        o = Out()
        o.y = pf.conv_pf(pf_in(pf, i["x"]), i["wp"], i["b"], ksize=ks, stride=stride, rowbias=i["rb"], resid=pf_in(pf, i["res"]))
        o.y2 = pf.conv_pf(pf_in(pf, i["x"]), i["wp"], None, ksize=ks, stride=stride)
        return o.add(pf_out(o.y), "full.").add(pf_out(o.y2), "bare.")

    c = three_ways(G, case, inp)
    ref = F.conv2d(inp["x"].float(), inp["w"].float(), inp["b"].float(), padding=ks // 2, stride=stride) + inp["rb"].float()[:, :, None, None] + inp["res"].float()
    assert _rel(c.y.to_nchw(), ref) <= TOL[dtype] and _zero_border(c.y)
    ref2 = F.conv2d(inp["x"].float(), inp["w"].float(), None, padding=ks // 2, stride=stride)
    assert (c.y2.to_nchw().float() - ref2).abs().max().item() <= TOL[dtype] * max(1.0, ref2.abs().max().item()) and _zero_border(c.y2)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_three_segment_launch_upsampler_direct_conv_out_and_input_packing(G, dtype):
    """conv3x3_res_pf (tests/test_gpu_pf.py:88, shape (2, 128, 320, 64, 128, 10, 6)), conv_up2x_pf (:283, (3, 5, 7, 64, 160)), gsw_conv3x3_pf_nchw and gsw_nchw_to_pf
    (tests/test_gpu_small.py:101-128, shapes (3, 64, 3, 5, 7), (2, 96, 8, 9, 4) and (3, 4, 8, 12), (2, 9, 5, 7))"""
    pf, N_, dt = G.pf, G.N, G.codec._dt(dtype)
    r = _rnd(17)
    h = lambda *s, scale=1.0: (r(*s) * scale).to(dtype).cuda()
    inp = dict(x=h(2, 128, 10, 6), w3=h(320, 128, 3, 3, scale=(9 * 128) ** -0.5), b=h(320), rb=h(2, 320), x1=h(2, 64, 10, 6), x2=h(2, 128, 10, 6),
               w1=h(320, 192, scale=192 ** -0.5), ux=h(3, 64, 5, 7), uw=h(160, 64, 3, 3, scale=(9 * 64) ** -0.5), ub=h(160, scale=0.1),
               ox=h(3, 64, 5, 7), ow=h(3, 64, 3, 3, scale=(9 * 64) ** -0.5), ob=h(3), px=h(2, 96, 9, 4), pw=h(8, 96, 3, 3, scale=(9 * 96) ** -0.5), pb=h(8),
               n1=h(3, 4, 8, 12), n2=h(2, 9, 5, 7))
    inp["wcat"] = torch.cat([pf.pack_conv_weight(inp["w3"]), inp["w1"]], dim=1).contiguous()
    inp.update(uw4=pf.pack_upsample_weight(inp["uw"]), owp=pf.pack_conv_weight(inp["ow"]), pwp=pf.pack_conv_weight(inp["pw"]))

    def case(i, L):
        o = Out()
        o.seg = pf.conv3x3_res_pf(pf_in(pf, i["x"]), i["wcat"], i["b"], rowbias=i["rb"], x1=pf_in(pf, i["x1"]), x2=pf_in(pf, i["x2"]))
        o.up = pf.conv_up2x_pf(pf_in(pf, i["ux"]), i["uw4"], i["ub"])
        o.add(pf_out(o.seg), "seg3.").add(pf_out(o.up), "up2x.")
        for nm, xk, wk, bk in (("nchw_a", "ox", "owp", "ob"), ("nchw_b", "px", "pwp", "pb")):
            B, C, H, W = i[xk].shape
            n_out = i[bk].numel()
            y = _alloc(L, (B, n_out, H, W), dtype)
            N_.check(G.lib.gsw_conv3x3_pf_nchw(pf_in(pf, i[xk]).rows.data_ptr(), i[wk].data_ptr(), i[bk].data_ptr(), y.data_ptr(), B, H, W, C, n_out, dt, None))
            o.written[nm] = y
        for nm in ("n1", "n2"):
            B, Cin, H, W = i[nm].shape
            p = pf.PF.empty(B, H, W, 64, dtype, "cuda")
            N_.check(G.lib.gsw_nchw_to_pf(i[nm].data_ptr(), p.rows.data_ptr(), B, Cin, H, W, 64, dt, None))
            o.add(pf_out(p), nm + ".")                                       # interior (channels past Cin zero), zero border, guard rows not this kernel's to write
            setattr(o, nm, p)
        return o

    c = three_ways(G, case, inp)
    f = lambda k: inp[k].float()
    ref = F.conv2d(f("x"), f("w3"), f("b"), padding=1) + f("rb")[:, :, None, None] + F.conv2d(torch.cat([inp["x1"], inp["x2"]], 1).float(), f("w1")[:, :, None, None])
    assert _rel(c.seg.to_nchw(), ref) <= TOL[dtype] and _zero_border(c.seg)
    refu = F.conv2d(F.interpolate(f("ux"), scale_factor=2.0, mode="nearest"), f("uw"), f("ub"), padding=1)
    assert (c.up.to_nchw().float() - refu).abs().max().item() <= (4e-3 if dtype == F16 else 3e-2) * max(1.0, refu.abs().max().item()) and _zero_border(c.up)
    assert _rel(c.written["nchw_a"], F.conv2d(f("ox"), f("ow"), f("ob"), padding=1)) <= TOL[dtype]
    assert _rel(c.written["nchw_b"], F.conv2d(f("px"), f("pw"), f("pb"), padding=1)) <= TOL[dtype]
    for nm in ("n1", "n2"):
        p, Cin = getattr(c, nm), inp[nm].shape[1]
        assert torch.equal(p.interior[..., :Cin], inp[nm].permute(0, 2, 3, 1)) and p.interior[..., Cin:].abs().max() == 0 and _zero_border(p)


def test_gn_only_convolution_record_fed_groupnorm_and_fallback(G):
    """conv_pf(gn_only=True) leaves the border unwritten; the record-fed GroupNorm does not read it, the statistics-pass fall-back zeroes it first.
    tests/test_gpu_gn_colstats.py:test_gn_only_convolution_skips_the_border_and_groupnorm_does_not_care, shape (8, 320, 320, 32, 32) and its bounds"""
    pf = G.pf
    B, C, N, H, W = 8, 320, 320, 32, 32
    r = _rnd(B + C + N)
    inp = dict(x=r(B, C, H, W).half().cuda(), w=(r(N, C, 3, 3) * (9 * C) ** -0.5).half().cuda(), b=r(N).half().cuda(), gamma=r(N).half().cuda(), beta=r(N).half().cuda())
    inp["wp"] = pf.pack_conv_weight(inp["w"])

    def case(i, L):
        with setting(pf, GN_FUSED_MAX_WGS=0, SPLITK_MAX=1):                   # as the fixture of test_gpu_gn_colstats.py: column records, no one-launch GroupNorm
            X = pf_in(pf, i["x"])
            y0 = pf.conv_pf(X, i["wp"], i["b"])
            assert y0.border_valid and y0.stats is not None
            y1 = pf.conv_pf(X, i["wp"], i["b"], gn_only=True)
            assert y1.stats is not None and not y1.border_valid
            st = y1.stats
            blocks = B * (H * W // st.rows)
            o = Out(written={"records": st.buf.view(st.npar, st.blocks, 2, N // 2)[:, :blocks]})
            o.add(pf_out(y0), "conv.").add(pf_out(y1, border=False), "gn_only.")          # checked now: the fall-back below writes the border
            if L is not None:
                for k, t in o.kept.items():
                    assert L.untouched(t) == t.numel(), k
                o.kept = {k: t for k, t in o.kept.items() if "border" not in k}
            ref = pf.groupnorm_pf(y0, i["gamma"], i["beta"], 32, 1e-5)
            out = pf.groupnorm_pf(y1, i["gamma"], i["beta"], 32, 1e-5)      # record-fed: gsw_groupnorm_pf_cs
            assert not y1.border_valid
            y1.stats = None
            out2 = pf.groupnorm_pf(y1, i["gamma"], i["beta"], 32, 1e-5)     # the statistics pass: zeroes the border first
            assert y1.border_valid
            o.add(pf_out(ref), "gn_ref.").add(pf_out(out), "gn_cs.").add(pf_out(out2), "gn_pass.")
            o.same["gn_only.rows_after_fallback"] = y1.rows
            o.y0, o.y1, o.ref, o.out, o.out2 = y0, y1, ref, out, out2
        return o

    c = three_ways(G, case, inp)
    assert torch.equal(c.y1.interior, c.y0.interior) and torch.equal(c.out.rows, c.ref.rows) and _zero_border(c.y1) and _zero_border(c.out)
    rr = F.silu(F.group_norm(c.y0.to_nchw().float(), 32, inp["gamma"].float(), inp["beta"].float(), 1e-5))
    assert (c.out2.to_nchw().float() - rr).abs().max().item() <= 2e-2 * max(1.0, rr.abs().max().item())
    assert (c.out.to_nchw().float() - rr).abs().max().item() <= 4e-3 * max(1.0, rr.abs().max().item())          # test_gpu_gn_colstats.py:86


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# norms and point-wise (tests/test_gpu_unet_fused.py, test_gpu_pf.py, test_gpu_small.py, test_gpu_xattn.py)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _gn_ref(x, gamma, beta, act, eps=1e-5):
    y = F.group_norm(x.float(), 32, gamma.float(), beta.float(), eps)
    return F.silu(y) if act else y


@pytest.mark.parametrize("dtype", [F16, BF16, torch.float32], ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("B,C,H,W", [(2, 64, 4, 2), (2, 1280, 8, 8), (2, 640, 32, 32)])
def test_groupnorm_silu_nchw(G, dtype, B, C, H, W):
    """tests/test_gpu_unet_fused.py:test_groupnorm_silu_vs_torch_fp32"""
    r = _rnd(C + H)
    inp = dict(x=(r(B, C, H, W) * 1.5 + 0.3).to(dtype).cuda(), gamma=(1 + 0.2 * r(C)).to(dtype).cuda(), beta=(0.2 * r(C)).to(dtype).cuda(), pb=(0.5 * r(B, C)).to(dtype).cuda())

    def case(i, L):
        return Out(written={"biased": G.codec.groupnorm_silu(i["x"], i["gamma"], i["beta"], 32, 1e-5, act=True, pre_bias=i["pb"]),
                            "plain": G.codec.groupnorm_silu(i["x"], i["gamma"], i["beta"], 32, 1e-5, act=False)})

    c = three_ways(G, case, inp)
    tol = {torch.float32: 2e-5, F16: 4e-3, BF16: 3e-2}[dtype]
    ref = _gn_ref(inp["x"].float() + inp["pb"].float()[:, :, None, None], inp["gamma"], inp["beta"], True)
    assert (c.written["biased"].float() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())
    ref = _gn_ref(inp["x"], inp["gamma"], inp["beta"], False)
    assert (c.written["plain"].float() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("B,C,C2,H,W", [(2, 64, 0, 4, 6), (3, 128, 0, 5, 7), (2, 1280, 0, 8, 8), (1, 128, 64, 5, 7), (2, 1280, 640, 16, 16), (2, 640, 0, 32, 32)])
def test_groupnorm_pf_fused_and_two_pass(G, dtype, B, C, C2, H, W):
    """groupnorm_pf / groupnorm_pf2: the one-launch kernel (gsw_groupnorm_pf_fused) and the statistics pass with its workspace, PF and token outputs.
    tests/test_gpu_pf.py:test_groupnorm_pf_vs_torch_fp32, tests/test_gpu_small.py:test_groupnorm_fused_vs_torch_fp32 (4e-3 fp16 / 3e-2 bf16)"""
    pf = G.pf
    r = _rnd(C + C2 + H)
    Ct = C + C2
    inp = dict(x=(r(B, C, H, W) * 1.5 + 0.3).to(dtype).cuda(), gamma=(1 + 0.2 * r(Ct)).to(dtype).cuda(), beta=(0.2 * r(Ct)).to(dtype).cuda())
    if C2:
        inp["x2"] = (r(B, C2, H, W) * 0.7 - 0.5).to(dtype).cuda()

    def case(i, L):
        o = Out()
        for nm, wgs in (("fused", 512), ("pass", 0)):
            with setting(pf, GN_FUSED_MAX_WGS=wgs, GN_FUSED_MAX_PIXELS=1 << 20):
                assert pf._gn_fused_ok(B, H, W, Ct, 32) == (wgs > 0)
                xp, xp2 = pf_in(pf, i["x"]), (pf_in(pf, i["x2"]) if C2 else None)
                y = pf.groupnorm_pf2(xp, xp2, i["gamma"], i["beta"], 32, 1e-5, act=True)
                o.add(pf_out(y), nm + ".")
                setattr(o, nm, y)
                if not C2:
                    o.written[nm + ".tokens"] = pf.groupnorm_pf(xp, i["gamma"], i["beta"], 32, 1e-5, act=False, tokens=True)
        return o

    c = three_ways(G, case, inp)
    tol = 4e-3 if dtype == F16 else 3e-2
    xx = inp["x"] if not C2 else torch.cat([inp["x"], inp["x2"]], dim=1)
    ref = _gn_ref(xx, inp["gamma"], inp["beta"], True)
    for nm in ("fused", "pass"):
        y = getattr(c, nm)
        assert (y.to_nchw().float() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item()) and _zero_border(y)
        if not C2:
            reft = _gn_ref(xx, inp["gamma"], inp["beta"], False).permute(0, 2, 3, 1).reshape(B, H * W, Ct)
            assert (c.written[nm + ".tokens"].float() - reft).abs().max().item() <= tol * max(1.0, reft.abs().max().item())


def test_groupnorm_from_column_records_concatenation_and_gn_proj_tokens(G):
    """gsw_groupnorm_pf_cs over the concatenation of two producers (tests/test_gpu_gn_colstats.py: 4e-3) and GroupNorm + proj_in as one launch with the
    statistics it leaves (tests/test_gpu_xattn.py:test_gn_proj_tokens_vs_fp32_reference, shape (3, 64, 64): 4e-3, allclose 2e-3)"""
    pf, xattn = G.pf, G.xattn
    B, H, W = 3, 64, 64
    r = _rnd(B * H + W)
    h = lambda *s, scale=1.0, off=0.0: (r(*s) * scale + off).half().cuda()
    inp = dict(src=h(B, 64, H, W, scale=1.5), cw=h(320, 64, 3, 3, scale=0.06), cb=h(320, scale=0.5), src2=h(B, 64, H, W), cw2=h(128, 64, 3, 3, scale=0.05),
               gamma=h(448, scale=0.2, off=1.0), beta=h(448, scale=0.2))
    inp.update(cwp=pf.pack_conv_weight(inp["cw"]), cwp2=pf.pack_conv_weight(inp["cw2"]))
    norm, lin = torch.nn.GroupNorm(32, 320, eps=1e-6), torch.nn.Linear(320, 320)
    with torch.no_grad():
        norm.weight.copy_(1.0 + 0.3 * r(320)); norm.bias.copy_(0.2 * r(320))
        lin.weight.copy_(r(320, 320) * 1.2 * 320 ** -0.5); lin.bias.copy_(0.2 * r(320))
    norm, lin = norm.half().cuda(), lin.half().cuda()

    def case(i, L):
        with setting(pf, GN_FUSED_MAX_WGS=0, SPLITK_MAX=1):
            x = pf.conv_pf(pf_in(pf, i["src"]), i["cwp"], i["cb"])
            x2 = pf.conv_pf(pf_in(pf, i["src2"]), i["cwp2"], None)
            assert pf._stats_usable(x) and pf._stats_usable(x2) and xattn.gn_proj_usable(x, norm, lin)
            y = xattn.gn_proj(x, norm, lin, eps_next=1e-5)
            cat = pf.groupnorm_pf2(x, x2, i["gamma"], i["beta"], 32, 1e-5, act=True)          # 448 / 32 = 14-channel groups: one straddles the two tensors
        o = Out(written={"tokens": y, "ostat": y._gsw_lnstat[0]}).add(pf_out(x), "x.").add(pf_out(x2), "x2.").add(pf_out(cat), "cat.")
        o.x, o.x2, o.cat = x, x2, cat
        return o

    c = three_ways(G, case, inp)
    xi = c.x.to_nchw().float()
    ref = F.linear(F.group_norm(xi, 32, norm.weight.float(), norm.bias.float(), norm.eps).permute(0, 2, 3, 1).reshape(B, H * W, 320), lin.weight.float(), lin.bias.float())
    y = c.written["tokens"]
    assert (y.float() - ref).abs().max().item() <= 4e-3 * max(1.0, ref.abs().max().item())
    yf = y.float()
    rstd = torch.rsqrt(yf.var(-1, unbiased=False) + 1e-5)
    assert torch.allclose(c.written["ostat"], torch.stack([rstd, -rstd * yf.mean(-1)], dim=-1).reshape(-1, 2), rtol=2e-3, atol=2e-3)
    refc = _gn_ref(torch.cat([c.x.to_nchw(), c.x2.to_nchw()], dim=1), inp["gamma"], inp["beta"], True)
    assert (c.cat.to_nchw().float() - refc).abs().max().item() <= 4e-3 * max(1.0, refc.abs().max().item()) and _zero_border(c.cat)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_add_layernorm_geglu_gather_rows(G, dtype):
    """add_layernorm at C in {8, 328, 648, 1288} x rows in {3, 9, 33}, with and without delta; geglu; gsw_gather_rows.
    tests/test_gpu_unet_fused.py (4e-3 / 3e-2; geglu 2e-3 / 1.6e-2), tests/test_gpu_small.py:test_gather_rows (equality)"""
    r = _rnd(5)
    shapes = [(rows, C) for C in (8, 328, 648, 1288) for rows in (3, 9, 33)]
    inp = {}
    for rows, C in shapes:
        inp.update({f"x{rows}_{C}": (r(rows, C) * 2 + 0.5).to(dtype).cuda(), f"d{rows}_{C}": r(rows, C).to(dtype).cuda()})
    for C in (8, 328, 648, 1288):
        inp.update({f"w{C}": (1 + 0.2 * r(C)).to(dtype).cuda(), f"b{C}": (0.2 * r(C)).to(dtype).cuda()})
    gshapes = [(5, 8, 16), (3, 77, 640), (1, 64, 10240)]
    for j, s in enumerate(gshapes):
        inp[f"g{j}"] = (r(*s) * 2).to(dtype).cuda()
    inp["table"] = r(1000, 20160).to(dtype).cuda()
    inp["idx_a"], inp["idx_b"] = torch.tensor([3, 999, 0, 500], device="cuda"), torch.tensor([1500, -4], device="cuda")
    inp["one"] = torch.full((), 77, device="cuda", dtype=torch.int64)

    def case(i, L):
        o = Out()
        for rows, C in shapes:
            k = f"{rows}_{C}"
            xn, y = G.codec.add_layernorm(i["x" + k], i["d" + k], i[f"w{C}"], i[f"b{C}"], 1e-5)
            x0, y0 = G.codec.add_layernorm(i["x" + k], None, i[f"w{C}"], i[f"b{C}"], 1e-5)
            assert x0 is i["x" + k]
            o.written.update({"sum" + k: xn, "ln" + k: y, "ln0" + k: y0})
        for j in range(len(gshapes)):
            o.written[f"geglu{j}"] = G.codec.geglu(i[f"g{j}"])
        rowb = 20160 * 2
        for nm, idx, per_row, n in (("gather_a", i["idx_a"], 1, 4), ("gather_b", i["idx_b"], 1, 2), ("gather_one", i["one"], 0, 3)):
            out = _alloc(L, (n, 20160), dtype)
            G.N.check(G.lib.gsw_gather_rows(i["table"].data_ptr(), rowb, 1000, idx.data_ptr(), per_row, out.data_ptr(), rowb, n, rowb, None))
            o.written[nm] = out
        return o

    c = three_ways(G, case, inp)
    tol = 4e-3 if dtype == F16 else 3e-2
    for rows, C in shapes:
        k = f"{rows}_{C}"
        xs = inp["x" + k] + inp["d" + k]
        assert torch.equal(c.written["sum" + k], xs)
        for nm, src in (("ln", xs), ("ln0", inp["x" + k])):
            ref = F.layer_norm(src.float(), (C,), inp[f"w{C}"].float(), inp[f"b{C}"].float(), 1e-5)
            assert (c.written[nm + k].float() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())
    for j in range(len(gshapes)):
        hh, gate = inp[f"g{j}"].float().chunk(2, dim=-1)
        ref = hh * F.gelu(gate)
        assert (c.written[f"geglu{j}"].float() - ref).abs().max().item() <= (2e-3 if dtype == F16 else 1.6e-2) * max(1.0, ref.abs().max().item())
    t = inp["table"]
    assert torch.equal(c.written["gather_a"], t[inp["idx_a"].clamp(0, 999)]) and torch.equal(c.written["gather_b"], t[inp["idx_b"].clamp(0, 999)])
    assert torch.equal(c.written["gather_one"], t[77].expand(3, -1))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# attention (tests/test_gpu_pf.py, test_gpu_small.py, test_gpu_gemm.py)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _attn_ref(q, k, v, H, valid=None):
    B, Sq, inner = q.shape
    D = inner // H
    if valid is not None:
        k, v = k[:, :valid], v[:, :valid]
    qf, kf, vf = (a.float().view(B, a.shape[1], H, D).transpose(1, 2) for a in (q, k, v))
    return (torch.softmax(qf @ kf.transpose(-1, -2) * D ** -0.5, dim=-1) @ vf).transpose(1, 2).reshape(B, Sq, inner)


# (B, heads, Sq, Sk, head_dim, valid_keys): the 128-query form, the 256-query form (more than 400 workgroups of 256 queries), the ragged shapes, padded contexts
# (K rows / V^T columns past valid_keys hold 50 / 1000 as tests/test_gpu_pf.py sets them), the LDS-DMA form at 1024 keys
ATTN = [(2, 5, 256, 256, 64, None), (21, 5, 1024, 1024, 64, None), (2, 5, 1, 8, 64, None), (1, 2, 200, 72, 80, None), (2, 8, 144, 144, 160, None),
        (2, 4, 144, 144, 40, None), (2, 3, 256, 128, 64, 1), (2, 3, 256, 128, 64, 77), (2, 20, 64, 128, 64, 77), (2, 3, 512, 1024, 64, 65),
        (2, 3, 512, 1024, 64, 999), (2, 8, 128, 128, 80, None)]


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("B,H,Sq,Sk,D,valid", ATTN)
def test_attention_forms_ragged_and_masked(G, dtype, B, H, Sq, Sk, D, valid):
    """tests/test_gpu_pf.py: 4e-3 fp16 / 2e-2 bf16 at the output's scale"""
    pf = G.pf
    r = _rnd(Sq + Sk + D + (valid or 0))
    q, k, v = (2.0 * r(B, Sq, H * D)).to(dtype).cuda(), r(B, Sk, H * D).to(dtype).cuda(), r(B, Sk, H * D).to(dtype).cuda()
    if valid is not None:
        k[:, valid:] = 50.0
        v[:, valid:] = 1000.0
    inp = dict(q=q, k=k, vt=v.transpose(1, 2).contiguous())

    def case(i, L):
        return Out(written={"out": pf.attention(i["q"], i["k"], i["vt"], H, valid_keys=valid)})

    c = three_ways(G, case, inp, ws_bytes=pf.SPLITK_BYTES)
    ref = _attn_ref(q, k, v, H, valid)
    tol = 4e-3 if dtype == F16 else 2e-2
    assert (c.written["out"].float() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("B,H,Sq,Sk,D", [(2, 3, 128, 2112, 64), (1, 8, 1024, 2304, 40), (1, 2, 256, 2752, 64)])
def test_attention_key_split_on_ledger_scratch(G, dtype, B, H, Sq, Sk, D):
    """gsw_attention_ws splitting the keys over several workgroups, partial results in pattern-filled scratch (tests/test_gpu_small.py:315, its bound)"""
    pf = G.pf
    r = _rnd(Sq + Sk + H)
    q, k, v = (2.0 * r(B, Sq, H * D)).to(dtype).cuda(), r(B, Sk, H * D).to(dtype).cuda(), r(B, Sk, H * D).to(dtype).cuda()
    inp = dict(q=q, k=k, vt=v.transpose(1, 2).contiguous())
    assert pf.ATTN_KEY_SPLIT

    def case(i, L):
        return Out(written={"out": pf.attention(i["q"], i["k"], i["vt"], H)})

    c = three_ways(G, case, inp, ws_bytes=pf.SPLITK_BYTES)
    with setting(pf, ATTN_KEY_SPLIT=False):
        unsplit = pf.attention(q, k, inp["vt"], H)
    ref = _attn_ref(q, k, v, H)
    tol = (4e-3 if dtype == F16 else 2e-2) * max(1.0, ref.abs().max().item())
    a = c.written["out"]
    assert (a.float() - ref).abs().max().item() <= tol and (a.float() - unsplit.float()).abs().max().item() <= tol
    assert not torch.equal(a, unsplit) or dtype == BF16                       # the split path really ran (test_gpu_small.py:342)


def test_attention_column_slices_and_two_launches_into_one_output(G):
    """q and k as column slices of a fused projection; two launches into the two halves of one `out` (unet.py: the guidance halves): each leaves the other
    half untouched.  Bound of tests/test_gpu_pf.py (4e-3)."""
    pf = G.pf
    B, H, S, D = 2, 5, 256, 64
    inner = H * D
    r = _rnd(9)
    qk = r(B, S, 2 * inner).half().cuda()
    qk[..., :inner] *= 2.0
    v, v2 = r(B, S, inner).half().cuda(), r(B, S, inner).half().cuda()
    inp = dict(qk=qk, vt=v.transpose(1, 2).contiguous(), vt2=v2.transpose(1, 2).contiguous())

    def case(i, L):
        q, k = i["qk"][..., :inner], i["qk"][..., inner:]
        o = _alloc(L, (2 * B, S, inner), F16)
        pf.attention(q, k, i["vt"], H, out=o[:B])
        if L is not None:
            torch.cuda.synchronize()
            assert L.untouched(o[B:]) == o[B:].numel() and L.untouched(o[:B]) == 0, "the first launch wrote outside its half of `out`"
        first = o[:B].clone()
        pf.attention(q, k, i["vt2"], H, out=o[B:])
        res = Out(written={"out": o, "sliced": pf.attention(q, k, i["vt"], H)})
        assert torch.equal(o[:B], first), "the second launch touched the first half of `out`"
        return res

    c = three_ways(G, case, inp)
    q, k = qk[..., :inner], qk[..., inner:]
    ref = torch.cat([_attn_ref(q, k, v, H), _attn_ref(q, k, v2, H)], dim=0)
    assert (c.written["out"].float() - ref).abs().max().item() <= 4e-3 * max(1.0, ref.abs().max().item())
    assert torch.equal(c.written["sliced"], c.written["out"][:B])


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_single_head_attention_and_row_softmax_with_ld(G, engine, dtype):
    """attention_single_head (scores buffer, zero-padded key axis) and softmax_rows_ on a column slice (ld > cols): tests/test_gpu_gemm.py:156-179"""
    pf = engine
    r = _rnd(3)
    sm = [(7, 8), (5, 1000), (300, 4096)]
    inp = {f"s{j}": (4.0 * r(rows, cols + 8)).to(dtype).cuda() for j, (rows, cols) in enumerate(sm)}
    ah = [(2, 48, 128), (3, 64, 64)] if dtype == F16 else []
    for j, (B, S, d) in enumerate(ah):
        inp[f"qk{j}"], inp[f"v{j}"] = r(B, S, 2 * d).to(dtype).cuda(), r(B, S, d).to(dtype).cuda()
        inp[f"vt{j}"] = inp[f"v{j}"].transpose(1, 2).contiguous()

    def case(i, L):
        o = Out()
        for j, (rows, cols) in enumerate(sm):
            x = i[f"s{j}"] if L is not None else i[f"s{j}"].clone()          # in place: the clean run works on a copy
            pf.softmax_rows_(x[:, :cols], 0.37)
            o.same[f"softmax{j}"] = x                                         # the whole buffer: columns past `cols` must come out as they went in
        for j, (B, S, d) in enumerate(ah):
            o.written[f"single{j}"] = pf.attention_single_head(i[f"qk{j}"][..., :d], i[f"qk{j}"][..., d:], i[f"vt{j}"])
        return o

    c = three_ways(G, case, inp)
    for j, (rows, cols) in enumerate(sm):
        x, keep = c.same[f"softmax{j}"], inp[f"s{j}"]
        ref = torch.softmax(0.37 * keep[:, :cols].float(), dim=-1)
        assert (x[:, :cols].float() - ref).abs().max().item() <= (2e-3 if dtype == F16 else 1.6e-2) * ref.max().item() + 1e-6
        assert torch.equal(x[:, cols:], keep[:, cols:])
    for j, (B, S, d) in enumerate(ah):
        qf, kf, vf = inp[f"qk{j}"][..., :d].float(), inp[f"qk{j}"][..., d:].float(), inp[f"v{j}"].float()
        ref = torch.softmax(qf @ kf.transpose(1, 2) * d ** -0.5, dim=-1) @ vf
        assert (c.written[f"single{j}"].float() - ref).abs().max().item() <= 6e-3 * max(1.0, ref.abs().max().item())


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the cross-attention launch (tests/test_gpu_xattn.py)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _stat(x, eps):
    xf = x.float()
    rstd = torch.rsqrt(xf.var(-1, unbiased=False) + eps)
    return torch.stack([rstd, -rstd * xf.mean(-1)], dim=-1).reshape(-1, 2).contiguous()


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("xB,oB,S,shared,pre", [(3, 3, 128, True, False), (2, 4, 384, False, False), (2, 4, 384, False, True), (2, 2, 128, False, True)])
def test_xattn_fused_and_pre(G, dtype, xB, oB, S, shared, pre):
    """xattn.fused and its pre_o= form, one context stream / the CFG index over shared latents; `ostat` is written in full.
    tests/test_gpu_xattn.py:_case / _pre_case: 4e-3 fp16, 3e-2 bf16; statistics allclose 2e-3"""
    from test_xattn_host import _module, reference
    xattn = G.xattn
    heads, seed = 5, 82 + S
    attn, norm = _module(heads, 64, 1024, dtype, seed)
    attn, norm = attn.cuda(), norm.cuda()
    g = torch.Generator().manual_seed(seed + 100)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = (rn(xB, S, 320) * 1.3 + 0.4).to(dtype).cuda()
    ctx = rn(1, 77, 1024).to(dtype).cuda().expand(oB, -1, -1) if shared else rn(oB, 77, 1024).to(dtype).cuda()
    blob, uv, idx = xattn.context_operands(attn, norm, ctx, dtype)
    inp = dict(x=x, blob=blob, uv=uv, stat=_stat(x, norm.eps))
    if idx is not None:
        inp["idx"] = idx
    if pre:
        lin = torch.nn.Linear(320, 320)
        with torch.no_grad():
            lin.weight.copy_(rn(320, 320) * 1.2 * 320 ** -0.5); lin.bias.copy_(0.2 * rn(320))
        lin = lin.to(dtype).cuda()
        inp.update(o=rn(xB, S, 320).to(dtype).cuda(), pw=xattn.out_projection_operand(lin, dtype))

    def case(i, L):
        if pre:
            y = xattn.fused(i["x"], None, i["blob"], i["uv"], i.get("idx"), oB, heads, eps_out=1e-5, pre_o=i["o"], pre_w=i["pw"], pre_eps=norm.eps)
        else:
            y = xattn.fused(i["x"], i["stat"], i["blob"], i["uv"], i.get("idx"), oB, heads, eps_out=1e-5)
        return Out(written={"y": y, "ostat": y._gsw_lnstat[0]})

    c = three_ways(G, case, inp)
    x1 = (x.float() + F.linear(inp["o"].float(), lin.weight.float(), lin.bias.float())).to(dtype) if pre else x
    want = torch.cat([reference(x1, norm, attn, ctx[j * xB:(j + 1) * xB]) for j in range(oB // xB)], dim=0)
    y = c.written["y"]
    assert (y.float() - want).abs().max().item() <= (4e-3 if dtype == F16 else 3e-2) * max(1.0, want.abs().max().item())
    assert torch.allclose(c.written["ostat"], _stat(y, 1e-5), rtol=2e-3, atol=2e-3)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# codec and loops (tests/test_gpu_codec.py, test_gpu_trace.py, test_gpu_trace_keyed.py): equality with the oracle
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_keystream_embed_and_uniform_streams(G):
    import gs_oracle as O
    from test_gpu_codec import _check_exact          # at most one fp32 ulp from the fp64 oracle's latent
    codec = G.codec
    lattices = [((4, 17, 25), 4), ((4, 8, 8), 32), ((4, 1, 1), 1)]
    inp = {}
    for j, (shape, mb) in enumerate(lattices):
        inp[f"u{j}"] = torch.from_numpy(np.random.RandomState(j).uniform(0, 1, (2, int(np.prod(shape))))).cuda()
    msgs = [bytes(np.random.RandomState(mb).randint(0, 256, mb, dtype=np.uint8)) for _, mb in lattices]          # tests/test_gpu_codec.py:191

    def case(i, L):
        o = Out()
        for n in (1, 63, 65, 1001):
            o.written[f"ks{n}"] = codec.keystream(KEY, NONCE, n)
        for j, (shape, mb) in enumerate(lattices):
            o.written[f"z{j}"] = codec.embed_batch(KEY, NONCE, msgs[j], 2, shape, u=i[f"u{j}"])
        for n in (1, 311, 313, 16384 + 7):
            o.written[f"philox{n}"] = codec.philox_uniform(0xDEADBEEFCAFE, 5, 2, n)
            o.written[f"mt{n}"] = codec.mt19937_uniform(n, np.random.RandomState(n))
        return o

    c = three_ways(G, case, inp)
    for n in (1, 63, 65, 1001):
        assert c.written[f"ks{n}"].cpu().numpy().tobytes() == O.chacha20_keystream(KEY, NONCE, n)
    for j, (shape, mb) in enumerate(lattices):
        u = inp[f"u{j}"].cpu().numpy()
        _check_exact(c.written[f"z{j}"].cpu().numpy(), np.stack([O.embed_latent(msgs[j], KEY, NONCE, u[b], shape) for b in range(2)]))
    for n in (1, 311, 313, 16384 + 7):
        np.testing.assert_array_equal(c.written[f"philox{n}"].cpu().numpy(), O.philox_uniform(0xDEADBEEFCAFE, 5, 2, n))
        np.testing.assert_array_equal(c.written[f"mt{n}"].cpu().numpy(), np.random.RandomState(n).random_sample(n))


@pytest.mark.parametrize("dtype", [F16, BF16, torch.float32, torch.float64], ids=["f16", "bf16", "f32", "f64"])
def test_extract_bit_matches_sign_pack(G, dtype):
    import gs_oracle as O
    codec = G.codec
    cases = [((4, 64, 64), 256), ((4, 17, 25), 8), ((4, 1, 1), 2)]
    inp = {}
    for j, (shape, ml) in enumerate(cases):
        n = int(np.prod(shape))
        z = torch.from_numpy(np.clip(np.random.RandomState(n + ml).standard_normal((3, n)).astype(np.float32) * 1.5, -8, 8)).to(dtype)
        z[1].mul_(0)
        inp[f"z{j}"] = z.cuda()
    g = torch.Generator().manual_seed(1)
    inp["s0"] = torch.randn(2, 1, 1, 8, generator=g, dtype=torch.float64).to(dtype).cuda()
    inp["s1"] = torch.randn(4, 4, 13, 10, generator=g, dtype=torch.float64).to(dtype).cuda()
    msg = O.pad_message("lthero", 32)

    def case(i, L):
        o = Out()
        for j, (shape, ml) in enumerate(cases):
            bits, flags, counts = codec.extract_batch(i[f"z{j}"], KEY, NONCE, ml, return_counts=True)
            o.written.update({f"bits{j}": bits, f"flags{j}": flags, f"counts{j}": counts})
        o.written["matches"] = codec.bit_matches(o.written["bits0"], 256, msg)
        for k in ("s0", "s1"):
            signs, flags = codec.sign_pack(i[k])
            o.written.update({k + ".signs": signs, k + ".flags": flags})
        return o

    c = three_ways(G, case, inp)
    for j, (shape, ml) in enumerate(cases):
        zz = inp[f"z{j}"].cpu().to(torch.float64).numpy()
        bits = c.written[f"bits{j}"].cpu().numpy()
        for b in range(3):
            got = codec.bits_to_str(bits[b])
            assert got[:ml] == O.recover_bits(zz[b], KEY, NONCE, ml) and set(got[ml:]) <= {"0"}
        assert int(c.written[f"flags{j}"].abs().sum()) == 0
    bits0 = c.written["bits0"].cpu().numpy()
    want = [sum(a == b for a, b in zip(codec.bits_to_str(bits0[b_]), codec.bits_to_str(msg))) for b_ in range(3)]
    assert c.written["matches"].cpu().tolist() == want
    for k in ("s0", "s1"):
        z64 = inp[k].cpu().double().numpy().reshape(inp[k].shape[0], -1)
        assert np.array_equal(c.written[k + ".signs"].cpu().numpy(), np.stack([np.packbits(O.quantise(z64[b]).astype(np.uint8)) for b in range(z64.shape[0])]))
        assert int(c.written[k + ".flags"].abs().sum()) == 0


@pytest.mark.parametrize("dtype", [F16, BF16, torch.float32], ids=["f16", "bf16", "f32"])
def test_ddim_steps(G, dtype):
    """tests/test_gpu_codec.py:335-371: ddim_step / _cfg against fp32 torch, ddim_step_extract against the unfused pair"""
    import gs_oracle as O
    codec = G.codec
    a, b = O.ddim_coefficients(O.sd_alphas_cumprod()[1], O.sd_alphas_cumprod()[21])
    r = _rnd(4)
    inp = {}
    for n in (7, 8, 1001):
        inp.update({f"x{n}": r(n).to(dtype).cuda(), f"e{n}": r(n).to(dtype).cuda(), f"t{n}": r(n).to(dtype).cuda()})
    inp.update(zx=r(4, 4, 17, 25).to(dtype).cuda(), ze=r(4, 4, 17, 25).to(dtype).cuda())
    for n in (7, 8, 1001):
        inp.update({f"fx{n}": r(2, n).to(dtype).cuda(), f"fe{n}": r(2, n).to(dtype).cuda()})

    def case(i, L):
        o = Out()
        for n in (7, 8, 1001):
            o.written[f"step{n}"] = codec.ddim_step(i[f"x{n}"], i[f"e{n}"], float(a), float(b))
            o.written[f"cfg{n}"] = codec.ddim_step_cfg(i[f"x{n}"], i[f"e{n}"], i[f"t{n}"], float(a), float(b), 7.5)
            # the fused last step on two images of n elements (7 and 1001: the vote pads the lattice to whole bytes)
            zo = _alloc(L, (2, n), dtype)
            bits, flags, counts = codec.ddim_step_extract(i[f"fx{n}"], i[f"fe{n}"], 1.0123, -0.0456, KEY, NONCE, 8, z_out=zo, return_counts=True)
            o.written.update({f"z{n}": zo, f"bits{n}": bits, f"flags{n}": flags, f"counts{n}": counts})
        zo = _alloc(L, (4, 4, 17, 25), dtype)
        bits, flags, counts = codec.ddim_step_extract(i["zx"], i["ze"], 1.0123, -0.0456, KEY, NONCE, 8, z_out=zo, return_counts=True)
        o.written.update(z=zo, bits=bits, flags=flags, counts=counts)
        return o

    c = three_ways(G, case, inp)
    tol = {torch.float32: 5e-7, F16: 1e-3, BF16: 8e-3}[dtype]
    a32, b32 = float(np.float32(a)), float(np.float32(b))
    for n in (7, 8, 1001):
        x, e, t = inp[f"x{n}"].float(), inp[f"e{n}"].float(), inp[f"t{n}"].float()
        ref = a32 * x + b32 * e
        assert (c.written[f"step{n}"].float() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())
        ref2 = a32 * x + b32 * (e + 7.5 * (t - e))
        assert (c.written[f"cfg{n}"].float() - ref2).abs().max().item() <= 8 * tol * max(1.0, ref2.abs().max().item())
    for sfx, xk, ek in [("", "zx", "ze")] + [(str(n), f"fx{n}", f"fe{n}") for n in (7, 8, 1001)]:
        z = codec.ddim_step(inp[xk], inp[ek], 1.0123, -0.0456)
        bits0, flags0, cnt0 = codec.extract_batch(z, KEY, NONCE, 8, return_counts=True)
        assert torch.equal(c.written["z" + sfx], z), f"{int((c.written['z' + sfx] != z).sum())} elements of the fused step's latent differ from gsw_ddim_step's"
        assert torch.equal(c.written["bits" + sfx], bits0) and torch.equal(c.written["flags" + sfx], flags0) and torch.equal(c.written["counts" + sfx], cnt0)


def test_registry_searches(G):
    """trace_topk and trace_keyed_topk with a registry size off the tile and k > 1, the registry / the records wrapped: equality with the host searches
    (tests/test_gpu_trace.py:_check, tests/test_gpu_trace_keyed.py:test_keyed_search_matches_oracle_codewords)"""
    from gswm_amd import trace as T
    from test_gpu_trace import _case
    from test_gpu_trace_keyed import _records_and_codewords, _rows
    codec = G.codec
    U, M, B, V = 63, 200, 64, 64
    counts, reg = _case(U, M, B, V, seed=U + M)
    Uk, n, mb, Bk, k = 63, 520, 5, 64, 8
    rng = np.random.default_rng(Uk * 7 + n + mb + Bk)
    recs, cw = _records_and_codewords(rng, Uk, n, mb)
    signs = rng.integers(0, 256, (Bk, n // 8), dtype=np.uint8)
    signs[0], signs[-1], signs[1] = 0x00, 0xFF, cw[Uk // 2]
    inp = dict(counts=torch.from_numpy(counts).cuda(), reg=torch.from_numpy(reg).cuda(), signs=torch.from_numpy(signs).cuda(), rows=_rows(T, recs, mb).to_device())

    def case(i, L):
        idx, score = codec.trace_topk(i["counts"], V, i["reg"], k=4, soft=True)
        hidx, hscore = codec.trace_topk(i["counts"], V, i["reg"], k=4, soft=False)
        kidx, kscore = codec.trace_keyed_topk(i["signs"], n, i["rows"], mb, k=k)
        return Out(written=dict(idx=idx, score=score, hidx=hidx, hscore=hscore, kidx=kidx, kscore=kscore))

    c = three_ways(G, case, inp)
    for soft, a, b in ((True, "idx", "score"), (False, "hidx", "hscore")):
        want_idx, want_score = T.topk_host(counts, V, reg, 4, soft)
        assert np.array_equal(c.written[b].cpu().numpy(), want_score) and np.array_equal(c.written[a].cpu().numpy(), want_idx)
    want_idx, want_score = T.keyed_topk_host(signs, cw, k)
    assert np.array_equal(c.written["kscore"].cpu().numpy(), want_score) and np.array_equal(c.written["kidx"].cpu().numpy(), want_idx)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# image stages (tests/test_gpu_image.py, test_gpu_geom.py): uint8 outputs, (c) and equality with the oracle / Pillow carry the check
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_image_stages_against_the_oracle(G):
    import image_oracle as IO
    from test_gpu_image import batch
    im = G.imaging
    resize = [((37, 41), (41, 37)), ((9, 7), (3, 2)), ((5, 5), (40, 1)), ((64, 48), (100, 37))]
    jpeg = [(1, 1), (2, 3), (17, 16), (33, 513)]
    blur = [((1, 7), 3), ((20, 3), 1.7), ((20, 3), 10), ((33, 47), 3)]
    host, inp = {}, {}
    for j, (hw, size) in enumerate(resize):
        host[f"r{j}"] = batch(*hw, 2, seed=hw[0] + size[0])
    for j, hw in enumerate(jpeg):
        host[f"j{j}"] = batch(*hw, 2, seed=hw[0] * 131 + hw[1])
    for j, (hw, rad) in enumerate(blur):
        host[f"b{j}"] = batch(*hw, 2, seed=hw[0] + 7)
    host["p"] = batch(33, 47, 2, seed=9)
    g = torch.Generator().manual_seed(0)
    for k, v in host.items():
        inp[k] = torch.from_numpy(v).cuda()
    tens = {dt: torch.rand(2, 3, 24, 40, generator=g).to(dt) for dt in (F16, BF16, torch.float32)}
    lat = (torch.randn(2, 3, 24, 40, generator=g) * 1.5).half()
    inp.update({f"t{j}": t.cuda() for j, t in enumerate(tens.values())}, lat=lat.cuda())

    def case(i, L):
        o = Out()
        for j, (hw, size) in enumerate(resize):
            o.written[f"resize{j}"] = im.resize_lanczos(i[f"r{j}"], size)
            o.written[f"resize{j}.f16"] = im.resize_lanczos(i[f"r{j}"], size, out="f16")
        for j in range(len(tens)):
            o.written[f"toimg{j}"] = im.tensor_to_image(i[f"t{j}"])
        o.written["toimg.lat"] = im.tensor_to_image(i["lat"], denormalise=True)
        for j, hw in enumerate(jpeg):
            for q in (10, 75):
                o.written[f"jpeg{j}q{q}"] = im.jpeg_roundtrip(i[f"j{j}"], q)
        for j, (hw, rad) in enumerate(blur):
            o.written[f"blur{j}"] = im.gaussian_blur(i[f"b{j}"], rad)
        for op, s in (("brightness", 0.3), ("brightness", 1.7), ("contrast", 0.3), ("contrast", 5.0), ("invert", 0.0), ("togray", 0.0), ("horizontal_flip", 0.0),
                      ("vertical_flip", 0.0)):
            o.written[f"{op}{s}"] = im.pointwise(i["p"], op, s)
        o.written["noise"] = im.pointwise(i["p"], "noise", 0.1, seed=5)
        return o

    c = three_ways(G, case, inp)
    w = {k: v.cpu().numpy() for k, v in c.written.items()}
    for j, (hw, size) in enumerate(resize):
        for b in range(2):
            ref = IO.resize_lanczos(host[f"r{j}"][b], size)
            assert np.array_equal(w[f"resize{j}"][b], ref) and np.array_equal(w[f"resize{j}.f16"][b], IO.normalise_like_reference(ref))
    for j, t in enumerate(tens.values()):
        assert np.array_equal(w[f"toimg{j}"], (t.permute(0, 2, 3, 1).float().numpy() * 255).round().astype("uint8"))
    assert np.array_equal(w["toimg.lat"], ((lat / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).float().numpy() * 255).round().astype("uint8"))
    for j, hw in enumerate(jpeg):
        for q in (10, 75):
            for b in range(2):
                assert np.array_equal(w[f"jpeg{j}q{q}"][b], IO.jpeg_roundtrip(host[f"j{j}"][b], q)), (hw, q)
    for j, (hw, rad) in enumerate(blur):
        for b in range(2):
            assert np.array_equal(w[f"blur{j}"][b], IO.gaussian_blur(host[f"b{j}"][b], rad)), (hw, rad)
    p = host["p"]
    for b in range(2):
        for f in (0.3, 1.7):
            assert np.array_equal(w[f"brightness{f}"][b], IO.enhance_brightness(p[b], f))
        for f in (0.3, 5.0):
            assert np.array_equal(w[f"contrast{f}"][b], IO.enhance_contrast(p[b], f))
        assert np.array_equal(w["togray0.0"][b], IO.rgb_to_l(p[b])[..., None].repeat(3, axis=2))
    assert np.array_equal(w["invert0.0"], 255 - p) and np.array_equal(w["horizontal_flip0.0"], p[:, :, ::-1]) and np.array_equal(w["vertical_flip0.0"], p[:, ::-1])


@pytest.mark.parametrize("hw", [(1, 7), (7, 1), (33, 95)])
def test_geometric_attacks_against_pillow(G, hw):
    """affine_nearest (rotation), crop_resize (resizedcrop) and box_mask (erasing, randomcrop) through distortions.apply_distortion, per-image seeds:
    tests/test_gpu_geom.py:test_geometric_types_equal_pillow_per_image_seeds"""
    from gswm_amd import distortions as D
    from test_gpu_geom import GEOM, pil_reference, synth
    B, seed = 3, 33
    imgs = np.stack([synth(*hw, seed=100 * B + k) for k in range(B)])
    inp = dict(dev=torch.from_numpy(imgs).cuda())
    rels = (0.0, 0.3, 0.77, 1.0)

    def case(i, L):
        return Out(written={f"{t}{r}": D.apply_distortion(i["dev"], t, r, distortion_seed=seed) for t in GEOM for r in rels})

    c = three_ways(G, case, inp)
    for t in GEOM:
        for r in rels:
            got = c.written[f"{t}{r}"].cpu().numpy()
            s = D.relative_strength_to_absolute(r, t)
            for b in range(B):
                assert np.array_equal(got[b], pil_reference(imgs[b], t, s, seed + b)), (hw, t, r, b)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# whole models, eager (no graph capture): (a) and (c) against their own clean run; check() and release() per forward
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _model_three_ways(G, forward):
    with torch.no_grad():
        clean = forward()
        torch.cuda.synchronize()
        outs = []
        for pattern in (NAN, FINITE):
            L = Ledger(pattern)
            try:
                with poisoned(L):
                    y = forward()
                torch.cuda.synchronize()
                L.check()
                outs.append([t.clone() for t in y])
            finally:
                L.release()
    for a, n_, f_ in zip(clean, *outs):
        assert torch.isfinite(a.float()).all()
        assert torch.equal(_bits(n_), _bits(f_)), f"NAN and FINITE runs differ in {int((_bits(n_) != _bits(f_)).sum())} elements"
        assert torch.equal(_bits(a), _bits(n_)), f"poisoned runs differ from the clean run in {int((_bits(a) != _bits(n_)).sum())} elements"


def test_small_unet_forward(G):
    """the (64, 128, 128, 128) UNet of tests/test_gpu_pf.py:test_unet_own_attention_equals_sdpa_path"""
    U = G.unet
    m = U.synthetic_init_(U.UNet2DCondition(block_out_channels=(64, 128, 128, 128), cross_attention_dim=64, num_heads=(1, 2, 2, 2), head_dim=64), 0).cuda().half().eval()
    g = torch.Generator().manual_seed(0)
    x, c, t = torch.randn(2, 4, 64, 64, generator=g).cuda().half(), torch.randn(2, 77, 64, generator=g).cuda().half(), torch.tensor([981, 1]).cuda()
    _model_three_ways(G, lambda: (m(x, t, c),))


def test_sd21_shaped_unet_forward_one_image(G):
    """one image through the SD 2.1-shaped UNet with the small-batch kernels and automatic split-K (tests/test_gpu_splitk.py:188, tests/test_gpu_small.py:131)"""
    U = G.unet
    m = U.synthetic_init_(U.UNet2DCondition(), 0).cuda().half().eval()
    g = torch.Generator().manual_seed(3)
    x, c = torch.randn(1, 4, 64, 64, generator=g).cuda().half(), torch.randn(1, 77, 1024, generator=g).cuda().half()
    t = torch.full((), 481, dtype=torch.int64, device="cuda")
    U.FALLBACKS.clear()
    with setting(G.pf, SPLITK_MAX=0):
        _model_three_ways(G, lambda: (m(x, t, c),))
    assert U.FALLBACKS == {}, U.FALLBACKS


@pytest.mark.usefixtures("library_kernels_allowed")      # as tests/test_gpu_pf.py:test_vae_pf_path_equals_torch_path: small shapes off the hand-written path
def test_small_vae_encode_and_decode(G):
    """The (64, 128, 128, 128) VAE of tests/test_gpu_pf.py:test_vae_pf_path_equals_torch_path at its 64 x 48 image.  The encoder runs the PF kernels there and is
    held bit for bit.  The decoder does NOT: an 8 x 6 latent is off the padded-flat path (vae._pf_ok wants H, W multiples of 8), so `decode` runs the plain torch
    modules on library kernels, whose bits vary from run to run (measured: two poisoned runs of it differ in 13197 of 18432 elements by a few fp16 ulps) -- that
    path is compared with the bound of the existing test (2e-2 at the output's scale), and the decoder's own kernels are held bit for bit on an 8 x 8 latent."""
    V = G.vae
    v = V.synthetic_init_(V.AutoencoderKL(block_out_channels=(64, 128, 128, 128)), 3).cuda().half().eval()
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(2, 3, 64, 48, generator=g) * 2 - 1).cuda().half()
    z = torch.randn(2, 4, 8, 6, generator=g).cuda().half()
    z8 = torch.randn(2, 4, 8, 8, generator=g).cuda().half()
    assert V._pf_ok(x) and V._pf_ok(z8) and not V._pf_ok(z) and v.encoder._pf_shapes_ok() and v.decoder._pf_shapes_ok()
    _model_three_ways(G, lambda: (v.encode_mean(x), v.decode(z8)))
    with torch.no_grad():
        clean = v.decode(z)
        for pattern in (NAN, FINITE):
            L = Ledger(pattern)
            try:
                with poisoned(L):
                    y = v.decode(z)
                torch.cuda.synchronize()
                L.check()
                assert (y.float() - clean.float()).abs().max().item() <= 2e-2 * max(1.0, clean.float().abs().max().item())
            finally:
                L.release()
