"""GPU: the aligned registry search -- codec.counts_align bit for bit against the NumPy restatement of tests/trace_align_reference.py on poisoned, guard-banded
buffers (tests/poison.py) and against the device's own vote of the aligned latent, its refusals, the two searches against their restatement (ties and cuts
included), then trace_latents_aligned and trace_latents_keyed_aligned end to end on attacked, noisy latents, the tamper map under an alignment, and the front
end.  EXACT equality everywhere, no tolerance."""
import math
import os

import numpy as np
import pytest
import torch

import align_reference as AR
import key_search_reference as R
import trace_align_reference as TR
from poison import FINITE, NAN, Ledger, poisoned

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gswm_amd  # noqa: F401
    from gswm_amd import align, codec, detect, trace
    assert hasattr(codec, "counts_align")
    return codec, align, detect, trace


def _align_list(H, W, A):
    """identity first, then every legal d, with shifts that are zero, negative, >= the lattice's side and far outside it (all taken modulo)"""
    ds = [d for d in range(8) if H == W or not d & 1]
    shifts = [(0, 0), (-1, 2), (H, -W - 1), (H + 3, W + 5), (-2 * H - 1, 0), (0, 3 * W - 1), (1, 1), (-H // 2, W // 2)]
    out = [(0, 0, 0)]
    i = 1
    while len(out) < A:
        out.append((ds[i % len(ds)], *shifts[(i // len(ds) + i) % len(shifts)]))
        i += 1
    return out


def _key(rng):
    return bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))


# C, H, W, l, M, B, A: the smallest case; the byte path on a non-square lattice; two message words; three (not a power of two: one lane idles); 425-byte rows, odd
# W, the byte path; 70 images; V = 2048 on the byte path (eight copies per lane, 256 lanes per position); the longest message (64 message words); 648 alignments;
# V = 1 with 16 alignments per workgroup and a half-full last chunk (with 17 x 200 a workgroup takes 3 and the last chunk holds 2); a 32 KiB row
CASES = [(1, 8, 8, 1, 8, 1, 1), (3, 5, 8, 1, 24, 3, 4), (4, 16, 16, 1, 64, 17, 200), (2, 6, 6, 4, 96, 3, 8), (4, 17, 25, 2, 200, 3, 12), (4, 12, 12, 2, 128, 70, 8),
         (4, 64, 64, 1, 8, 2, 8), (4, 64, 64, 4, 2048, 3, 8), (4, 64, 64, 1, 256, 2, 648), (1, 8, 8, 1, 64, 300, 120), (4, 128, 128, 4, 256, 1, 3)]


@pytest.mark.parametrize("C,H,W,l,M,B,A", CASES)
def test_counts_align_matches_the_restatement(G, C, H, W, l, M, B, A):
    codec = G[0]
    rng = np.random.default_rng(C + 3 * H + 7 * W + 11 * l + 13 * B + A + 17 * M)
    n_bits = C * H * W * l
    rows = rng.integers(0, 256, (B, n_bits // 8), dtype=np.uint8)
    key, nonce = _key(rng)
    aligns = _align_list(H, W, A)
    assert aligns[0] == (0, 0, 0) and len(aligns) == A
    want = TR.counts_align(rows, (C, H, W), l, aligns, R.keystreams([(key, nonce)], n_bits)[0], M)
    assert want.shape == (B, A, M) and (want.sum(axis=2) <= n_bits).all() and int(want.max()) <= n_bits // M
    r_dev = torch.from_numpy(rows).cuda()
    table = torch.tensor(aligns, dtype=torch.int32).cuda()
    for name, pattern in (("NAN", NAN), ("FINITE", FINITE)):
        L = Ledger(pattern)
        try:
            with poisoned(L):
                out = codec.counts_align(L.wrap(r_dev), (C, H, W), l, L.wrap(table) if pattern == NAN else aligns, key, nonce, M)     # a device table, a list
            torch.cuda.synchronize()
            L.check()
            assert L.untouched(out) == 0, f"never written ({name} run) -- {L.where(out)}"          # (no count is 0x7FFF7FFF or 0x4D4D4D4D)
            got = out.cpu().numpy()
        finally:
            L.release()
        assert got.dtype == np.int32 and got.shape == (B, A, M)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])


def test_counts_align_refuses_before_any_launch(G):
    codec = G[0]
    key, nonce = bytes(32), bytes(16)
    ok = torch.zeros(2, 8, dtype=torch.uint8).cuda()
    ident = [(0, 0, 0)]
    with pytest.raises(ValueError, match="524288"):
        codec.counts_align(ok, (4, 512, 512), 1, ident, key, nonce, 256)
    with pytest.raises(ValueError, match="multiple of 8"):
        codec.counts_align(ok, (1, 8, 8), 1, ident, key, nonce, 12)
    with pytest.raises(IndexError, match="string index out of range"):
        codec.counts_align(ok, (1, 8, 8), 1, ident, key, nonce, 24)
    with pytest.raises(ValueError, match="l must be"):
        codec.counts_align(ok, (1, 8, 8), 3, ident, key, nonce, 8)
    with pytest.raises(ValueError, match="0..7"):
        codec.counts_align(ok, (1, 8, 8), 1, [(8, 0, 0)], key, nonce, 8)
    with pytest.raises(ValueError, match="0..7"):
        codec.counts_align(ok, (1, 8, 8), 1, torch.tensor([[0, 0, 0], [-1, 0, 0]], dtype=torch.int32).cuda(), key, nonce, 8)
    with pytest.raises(ValueError, match="square"):
        codec.counts_align(ok, (1, 4, 16), 1, [(0, 0, 0), (3, 0, 0)], key, nonce, 8)
    with pytest.raises(ValueError, match="whole bytes"):
        codec.counts_align(torch.zeros(2, 2, dtype=torch.uint8).cuda(), (1, 3, 3), 1, ident, key, nonce, 8)
    with pytest.raises(ValueError, match="HIP device"):
        codec.counts_align(ok.cpu(), (1, 8, 8), 1, ident, key, nonce, 8)
    with pytest.raises(ValueError):
        codec.counts_align(ok, (1, 8, 16), 1, ident, key, nonce, 8)                                     # rows of 8 bytes, a lattice of 16
    with pytest.raises(ValueError):
        codec.counts_align(ok, (1, 8, 8), 1, ident, key[:31], nonce, 8)


@pytest.mark.parametrize("l", [1, 2, 4])
def test_counts_align_is_the_vote_of_the_aligned_latent(G, l):
    codec, AL = G[0], G[1]
    key, nonce = _key(np.random.default_rng(l))
    aligns = [(d, 0, 0) for d in range(4)] + [(d, -3, 5) for d in range(4, 8)]
    for dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        z = torch.randn(3, 4, 16, 16, generator=torch.Generator().manual_seed(l), dtype=torch.float64).to(dtype).cuda()
        packed, flags = codec.quant_pack(z, l)
        assert int(flags.abs().sum()) == 0
        out = codec.counts_align(packed, (4, 16, 16), l, aligns, key, nonce, 64)
        for i, a in enumerate(aligns):
            want = codec.extract_batch(AL.apply(z, a).contiguous(), key, nonce, 64, return_counts=True, l=l)[2]
            assert torch.equal(out[:, i], want), (l, dtype, a)


# ------------------------------------------------------------------------------------------------------------ the searches
@pytest.fixture(scope="module")
def SEARCH(G):
    """4 x 16 x 16, five noise images, 202 alignments of which the last two are the permutations of entries 0 and 100 written with a shift of the lattice's
    side, nine records of which rows 2 and 6 are the same (the registries refuse a repeated record, so row 6 is put in behind their backs); the restatement's
    scores, computed once"""
    codec, AL, D, T = G
    rng = np.random.default_rng(425)
    z = torch.randn(5, 4, 16, 16, generator=torch.Generator().manual_seed(425)).half()
    aligns = AL.alignments("d4", 2, 16, 16)
    assert aligns[100] == (4, 0, 0)
    aligns = aligns + [(0, 16, -16), (4, 0, 16)]
    key, nonce = _key(rng)
    msgs = [bytes(rng.integers(0, 256, 8, dtype=np.uint8)) for _ in range(9)]
    reg = T.Registry(8)
    for u, m in enumerate(msgs):
        reg.add(f"user-{u}", m)
    reg._messages[6] = reg._messages[2]
    reg._device_cache.clear()
    registry = np.stack([np.frombuffer(m, dtype=np.uint8) for m in reg._messages])
    _, S = TR.shared_scores(z, aligns, R.keystreams([(key, nonce)], 1024)[0], registry)
    records = [(*_key(rng), m) for m in msgs]
    kreg = T.KeyedRegistry(8)
    for u, r in enumerate(records):
        kreg.add(f"user-{u}", *r)
    records[6] = kreg._records[6] = records[2]
    kreg._device_cache.clear()
    return dict(z=z.cuda(), aligns=aligns, key=key, nonce=nonce, reg=reg, S=S, kreg=kreg, KS=TR.keyed_search(z, aligns, records))


def _found(results):
    return [[(c.index, c.alignment, c.score) for c in r.candidates] for r in results]


@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_the_searches_match_the_restatement(G, SEARCH, keyed, k):
    codec, AL, D, T = G
    S = SEARCH["KS" if keyed else "S"]
    aligns = SEARCH["aligns"]
    A = len(aligns)
    rec, al, sc = TR.merge(S, k)
    assert np.array_equal(S[:, :, 2], S[:, :, 6]) and np.array_equal(S[:, 0], S[:, 200]) and np.array_equal(S[:, 100], S[:, 201])       # the forced ties
    for order in rec.tolist():                                                       # row 6 never comes before row 2, a repeated alignment never wins
        assert 6 not in order or (2 in order and order.index(2) < order.index(6))
    assert (al < 200).all()
    want = [[(int(rec[b, j]), aligns[int(al[b, j])], int(sc[b, j])) for j in range(k)] for b in range(5)]
    per_image = 128 if keyed else 4 * 64                                             # bytes of one aligned image: its row, or its 64 counts
    name = "trace_keyed_topk" if keyed else "trace_topk"
    for budget, launches in ((None, 1), (2 * A * per_image, 3), (70 * per_image, 15)):     # one chunk; three chunks of images; the alignments of ONE image cut in three
        calls = []
        real = getattr(codec, name)
        setattr(codec, name, lambda *a, **kw: (calls.append(a[0].shape[0]), real(*a, **kw))[1])
        try:
            if keyed:
                got = T.trace_latents_keyed_aligned(SEARCH["z"], SEARCH["kreg"], aligns, k=k, budget_bytes=budget)
            else:
                got = T.trace_latents_aligned(SEARCH["z"], SEARCH["key"], SEARCH["nonce"], SEARCH["reg"], aligns, k=k, budget_bytes=budget)
        finally:
            setattr(codec, name, real)
        assert len(calls) == launches and sum(calls) == 5 * A, (budget, calls)
        assert _found(got) == want, (budget, _found(got), want)
        n = 1024
        for r in got:
            assert r.attributed is None and r.alignment is None                     # noise names nobody
            assert all(c.log10_p_any == T.log10_p_any(T.log10_p_soft(c.score, n), 9 * A) for c in r.candidates)


# ------------------------------------------------------------------------------------------------------------ end to end, one key
SATURATES_AT = 8.296875                 # the smallest fp16 at which float64 norm.cdf is 1.0: the reference cannot read such an element


@pytest.fixture(scope="module")
def E2E(G):
    codec, AL, D, T = G
    E = TR.SHARED
    s = TR.setup()
    cands = AL.alignments("d4", E["shift"], E["shape"][1], E["shape"][2])
    assert len(cands) == 200
    reg = T.Registry(E["msg_bytes"])
    for u, m in enumerate(s["registry"]):
        reg.add(f"user-{u}", bytes(m))
    counts, S = TR.shared_scores(s["z16"], cands, s["ks"], s["registry"])
    n = int(np.prod(E["shape"]))
    host = TR.trace_host(S, n, T.log10_p_soft, T.log10_p_any)
    # Noise of sigma 4 puts about 2 % of the elements at or past 8.296875, where the reference's cdf rounds to 1.0 and it raises for the whole image ("invalid
    # literal for int() with base 2"); the tracers refuse such an image as the reference does (asserted below on these very latents).  The device runs therefore
    # see the latents held just below that value: no sign changes, so every row, score and bound is still the restatement's of the unclipped latents.
    held = s["z16"].clamp(max=SATURATES_AT - 2.0 ** -7)
    assert float(s["z16"].max()) >= SATURATES_AT > float(held.max())
    assert np.array_equal(R.sign_rows(held.reshape(6, -1).double().numpy()), R.sign_rows(s["z16"].reshape(6, -1).double().numpy()))
    return dict(s, cands=cands, reg=reg, counts=counts, S=S, host=host, n=n, dev16=held.cuda())


def test_trace_latents_aligned_sees_through_flips_turns_and_shifts(G, E2E):
    codec, AL, D, T = G
    E = TR.SHARED
    limit = math.log10(E["fpr"])
    M, n, host, cands = 8 * E["msg_bytes"], E2E["n"], E2E["host"], E2E["cands"]
    print("log10 p over U A pairs:", [round(h[3], 1) for h in host])
    assert [h[0] for h in host] == list(E["rows"]) and all(h[3] <= limit for h in host)               # the restatement alone meets the case
    dev = T.trace_latents_aligned(E2E["dev16"], E2E["key"], E2E["nonce"], E2E["reg"], cands, fpr=E["fpr"])
    for b, (d, h) in enumerate(zip(dev, host)):
        top = d.candidates[0]
        assert d.attributed == f"user-{E['rows'][b]}" == top.user_id and len(d.candidates) == 1
        assert (top.index, top.score, top.log10_p_any) == (h[0], h[2], h[3]) and top.log10_p_any <= limit
        assert d.alignment == top.alignment == cands[h[1]] == AL.inverse(E["attacks"][b], 32, 32)
        restored = AL.apply(torch.from_numpy(E2E["attacked"][b]), d.alignment)
        assert torch.equal(restored, torch.from_numpy(E2E["clean"][b]))                                 # exactly the lattice as embedded
        voted = (2 * E2E["counts"][b, h[1]] > n // M).astype(np.uint8)                                  # the strict majority of the aligned row
        assert top.agree == int((voted == np.unpackbits(E2E["registry"][h[0]])).sum()) and top.agree > 32
        assert T.format_line("x.png", d, M).endswith(f", alignment: {AL.describe(d.alignment)}")
    # k = 3: the runners-up are other records, each with its own best alignment, none significant
    more = T.trace_latents_aligned(E2E["dev16"], E2E["key"], E2E["nonce"], E2E["reg"], cands, k=3, fpr=E["fpr"])
    rec, al, sc = TR.merge(E2E["S"], 3)
    for b, (d, one) in enumerate(zip(more, dev)):
        assert d.candidates[0] == one.candidates[0] and [(c.index, c.alignment, c.score) for c in d.candidates] == \
            [(int(rec[b, j]), cands[int(al[b, j])], int(sc[b, j])) for j in range(3)]
        assert all(c.log10_p_any > limit for c in d.candidates[1:])
    # the hard statistic runs and ranks the true row first
    _, Sh = TR.shared_scores(E2E["z16"], cands, E2E["ks"], E2E["registry"], soft=False)
    rec, al, sc = TR.merge(Sh, 1)
    hard = T.trace_latents_aligned(E2E["dev16"], E2E["key"], E2E["nonce"], E2E["reg"], cands, fpr=E["fpr"], soft=False)
    for b, d in enumerate(hard):
        top = d.candidates[0]
        assert (top.index, top.score) == (int(rec[b, 0]), int(sc[b, 0])) and top.index == E["rows"][b] and top.score == 2 * top.agree - M
        assert top.log10_p_any == T.log10_p_any(T.log10_p_hard(top.agree, M, n // M), 1000 * 200)
    # without alignments only the un-attacked image names its user
    plain = T.trace_latents(E2E["dev16"], E2E["key"], E2E["nonce"], E2E["reg"], fpr=E["fpr"])
    print("log10 p without alignments:", [round(r.candidates[0].log10_p_any, 1) for r in plain])
    assert [r.attributed for r in plain] == [f"user-{E['rows'][0]}"] + [None] * 5
    assert all(r.alignment is None and r.candidates[0].alignment is None and "alignment" not in T.format_line("x.png", r, M) for r in plain)


def test_unwatermarked_latents_name_nobody_and_flagged_ones_raise(G, E2E):
    codec, AL, D, T = G
    E = TR.SHARED
    cands = E2E["cands"]
    _, Sb = TR.shared_scores(E2E["blank"], cands, E2E["ks"], E2E["registry"])
    host = TR.trace_host(Sb, E2E["n"], T.log10_p_soft, T.log10_p_any)
    print("blank log10 p:", [round(h[3], 2) for h in host])
    assert all(h[3] > math.log10(E["fpr"]) for h in host)                                              # the restatement alone meets the case
    z = E2E["blank"].clone()
    z[3, 0, 0, 0] = float("nan")
    dev = T.trace_latents_aligned(z.cuda(), E2E["key"], E2E["nonce"], E2E["reg"], cands, fpr=E["fpr"], tamper_tile=8)
    for d, h in zip(dev[:3], host):
        top = d.candidates[0]
        assert d.attributed is None and d.alignment is None and d.tamper is None
        assert (top.index, top.alignment, top.score, top.log10_p_any) == (h[0], cands[h[1]], h[2], h[3])
    assert isinstance(dev[3], ValueError) and "NaN" in str(dev[3])
    # the six noisy latents as they are, saturated elements and all: the reference's error for every one of them, from both tracers, as from trace_latents
    raw = E2E["z16"].cuda()
    for out in (T.trace_latents_aligned(raw, E2E["key"], E2E["nonce"], E2E["reg"], cands), T.trace_latents(raw, E2E["key"], E2E["nonce"], E2E["reg"])):
        assert len(out) == 6 and all(isinstance(r, ValueError) and "invalid literal for int() with base 2" in str(r) for r in out)
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        T.trace_latents_aligned(E2E["blank"].view(4, -1).cuda(), E2E["key"], E2E["nonce"], E2E["reg"], cands)
    with pytest.raises(ValueError, match="square"):
        T.trace_latents_aligned(torch.zeros(1, 4, 16, 32).half().cuda(), E2E["key"], E2E["nonce"], E2E["reg"], cands)


# ------------------------------------------------------------------------------------------------------------ end to end, a key per record
def test_trace_latents_keyed_aligned_sees_through_flips_turns_and_shifts(G):
    codec, AL, D, T = G
    E = AR.E2E
    limit = math.log10(E["fpr"])
    s = TR.keyed_setup()
    cands = AL.alignments("d4", E["shift"], E["shape"][1], E["shape"][2])
    n = int(np.prod(E["shape"]))
    S = TR.keyed_search(s["z16"], cands, s["records"])
    host = TR.trace_host(S, n, T.log10_p_soft, T.log10_p_any)
    print("keyed log10 p over U A pairs:", [round(h[3], 1) for h in host])
    assert [h[0] for h in host] == list(s["rows"]) and all(h[3] <= limit for h in host)               # the restatement alone meets the case
    assert [cands[h[1]] for h in host] == [AL.inverse(a, 32, 32) for a in E["attacks"]]
    plain_host = TR.trace_host(S[:, :1], n, T.log10_p_soft, T.log10_p_any)
    assert [h[3] <= limit for h in plain_host] == [True] + [False] * 5
    reg = T.KeyedRegistry(E["msg_bytes"])
    for u, r in enumerate(s["records"]):
        reg.add(f"user-{u}", *r)
    z = s["z16"].cuda()
    dev = T.trace_latents_keyed_aligned(z, reg, cands, fpr=E["fpr"])
    for b, (d, h) in enumerate(zip(dev, host)):
        top = d.candidates[0]
        assert d.attributed == f"user-{s['rows'][b]}" and (top.index, top.score, top.log10_p_any) == (h[0], h[2], h[3])
        assert d.alignment == top.alignment == cands[h[1]]
        assert torch.equal(AL.apply(torch.from_numpy(s["attacked"][b]), d.alignment), torch.from_numpy(s["clean"][b]))
        assert top.agree == 8 * E["msg_bytes"]                                                          # sigma 1: every voted bit is the record's
    plain = T.trace_latents_keyed(z, reg, fpr=E["fpr"])
    assert [r.attributed for r in plain] == [f"user-{s['rows'][0]}"] + [None] * 5
    blank = T.trace_latents_keyed_aligned(s["blank"].cuda(), reg, cands, fpr=E["fpr"])
    assert all(r.attributed is None and r.alignment is None for r in blank)


# ------------------------------------------------------------------------------------------------------------ where, under an alignment
@pytest.mark.parametrize("keyed", [False, True])
def test_tamper_map_under_an_alignment(G, E2E, keyed):
    """The top 16 of the 32 lattice rows of image 1 are replaced by noise, THEN the image is mirrored: it is still attributed, and its map -- in the coordinates
    of the lattice as embedded -- marks intact tiles in the surviving lower half only and equals the map of the restatement's counts"""
    codec, AL, D, T = G
    from gswm_amd import tamper as TM
    E = TR.SHARED
    cands = E2E["cands"]
    z = torch.from_numpy(E2E["clean"][1]).clone()
    z[:, :16, :] = torch.randn(4, 16, 32, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    z16 = AL.apply(z, (4, 0, 0)).half()[None].contiguous()
    row = E["rows"][1]
    if keyed:
        reg = T.KeyedRegistry(E["msg_bytes"])
        reg.add("someone", bytes(range(32)), bytes(range(16)), bytes(8))
        reg.add("issuer", E2E["key"], E2E["nonce"], bytes(E2E["registry"][row]))
        (r,) = T.trace_latents_keyed_aligned(z16.cuda(), reg, cands, fpr=E["fpr"], tamper_tile=8)
        assert r.attributed == "issuer"
    else:
        (r,) = T.trace_latents_aligned(z16.cuda(), E2E["key"], E2E["nonce"], E2E["reg"], cands, fpr=E["fpr"], tamper_tile=8)
        assert r.attributed == f"user-{row}"
    assert r.alignment == (4, 0, 0) and r.tamper is not None and r.tamper.source == "registry"
    rows = R.sign_rows(z16.reshape(1, -1).double().numpy())
    back = AR.rows_align(rows, E["shape"], 1, [r.alignment])[0, 0]
    cw = E2E["ks"] ^ np.resize(E2E["registry"][row], E2E["n"] // 8)
    agree = TR.tile_agree(back, cw, E["shape"], 8)
    want = TM.make_map(agree, 4 * 64, 8, E["fpr"], "registry")
    assert np.array_equal(r.tamper.agree, agree) and np.array_equal(r.tamper.intact, want.intact)
    assert not r.tamper.intact[:2].any() and r.tamper.intact[2:].all()                                 # only the surviving half, and all of it (no noise was added)
    assert f", intact tiles 8/16, alignment: {AL.describe((4, 0, 0))}" in T.format_line("x.png", r, 64)


# ------------------------------------------------------------------------------------------------------------ front end
@pytest.mark.parametrize("keyed", [False, True])
def test_cli_with_align(G, E2E, keyed, tmp_path, monkeypatch, capsys):
    """The front end with --align d4 --align_shift 2 on two generated files.  Synthetic weights are not an autoencoder, so (as in test_gpu_align.py) the
    inversion is replaced by latents: the mirrored image and an unwatermarked one, and no model is built.  The rest -- registry, candidates from the lattice,
    search, trace.txt, the maps -- is the real run."""
    from PIL import Image
    from gswm_amd import extract as X
    codec, AL, D, T = G
    E = TR.SHARED
    d = tmp_path / "imgs"
    d.mkdir()
    rng = np.random.RandomState(5)
    for i in range(2):
        Image.fromarray(rng.randint(0, 256, (64, 64, 3), dtype=np.uint8)).save(str(d / f"img{i}.png"))
    mirrored = AL.apply(torch.from_numpy(E2E["clean"][1]), (4, 0, 0)).half()[None]
    latents = torch.cat([mirrored, E2E["blank"][:1]]).cuda()
    monkeypatch.setattr(X, "invert_decoded_images", lambda arrs, args, **kw: latents[:len(arrs)].clone())
    monkeypatch.setattr(X, "load_models", lambda *a, **kw: None)               # (nothing is inverted: building the synthetic UNet would be most of the test's time)
    reg_file = tmp_path / "registry.tsv"
    if keyed:
        reg = T.KeyedRegistry(E["msg_bytes"])
        for u in range(20):
            reg.add(f"user-{u}", E2E["key"] if u % 2 else bytes([u]) * 32, E2E["nonce"], bytes(E2E["registry"][E["rows"][1] - 7 + u]))
        extra = ["--per_record_keys"]
    else:
        reg = E2E["reg"]
        extra = ["--key_hex", E2E["key"].hex(), "--nonce_hex", E2E["nonce"].hex()]
    reg.save(reg_file)
    maps = tmp_path / "maps"
    T.main(["--images_directory_path", str(d), "--registry", str(reg_file), "--allow_synthetic_weights", "--num_inference_steps", "2", "--width", "256",
            "--height", "256", "--strict_kernels", "0", "--align", "d4", "--align_shift", "2", "--top", "2", "--tamper_map", str(maps)] + extra)
    out = capsys.readouterr().out
    lines = (d / "trace.txt").read_text().splitlines()
    start = lines.index("=" * 40 + "Batch Start" + "=" * 40)
    info = dict(l.split(",", 1) for l in lines[1:start])
    assert info["align"] == "d4" and info["align_shift"] == "2" and info["alignments"] == "200" and info["users"] == str(len(reg))
    assert lines[start + 1].startswith("SYNTHETIC WEIGHTS,")
    body = lines[start + 2:-1]
    files = X._DirJob(str(d)).files
    assert len(body) == len(files) == 2
    cands = AL.alignments("d4", 2, 32, 32)
    if keyed:
        want = T.trace_latents_keyed_aligned(latents, reg, cands, k=2, tamper_tile=8)
    else:
        want = T.trace_latents_aligned(latents, E2E["key"], E2E["nonce"], reg, cands, k=2, tamper_tile=8)
    for f, line, w in zip(files, body, want):
        assert line == T.format_line(os.path.basename(f), w, 64) and line in out
    user = "user-7" if keyed else f"user-{E['rows'][1]}"
    assert body[0].startswith(f"{os.path.basename(files[0])}, user: {user}, agreement, 1.0, log10 p, -") and body[0].endswith(", intact tiles 16/16, alignment: hflip")
    assert body[1].startswith(f"{os.path.basename(files[1])}, user: none, ") and "alignment" not in body[1]
    stem = os.path.splitext(os.path.basename(files[0]))[0]
    assert sorted(os.listdir(maps)) == [f"{stem}.tamper.npy", f"{stem}.tamper.png"]                    # the attributed image alone has a map
    with pytest.raises(SystemExit):
        T.main(["--images_directory_path", str(d), "--registry", str(reg_file), "--align", "d4", "--reliability", "7"] + extra)
