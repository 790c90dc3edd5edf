"""GPU: the alignment search -- codec.rows_align bit for bit against the NumPy restatement of tests/align_reference.py on poisoned, guard-banded
buffers (tests/poison.py) and against the device's own quantiser, its refusals, align.search_keys against its restatement (ties and chunking
included), then detect_latents(align=...) and align.extract_aligned end to end on attacked, noisy latents, and the front end.  EXACT equality
everywhere, no tolerance."""
import math
import os

import numpy as np
import pytest
import torch

import align_reference as AR
import key_search_reference as R
from poison import FINITE, NAN, Ledger, poisoned

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gswm_amd  # noqa: F401
    from gswm_amd import align, codec, detect, trace
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


def _by_chance(want, pattern):
    """how many bytes of the expected output equal the pattern's byte at their place (its low byte sits at even offsets): exactly those look untouched"""
    flat = want.reshape(-1)
    return int((flat[0::2] == (pattern & 0xFF)).sum() + (flat[1::2] == (pattern >> 8)).sum())


# C, H, W, l, B, A.  The issue's table; then a row of 65 536 bytes (the longest that is staged in LDS; not square: the four flips) and the first past it (read
# in place, odd W), the largest lattice (read in place), and 300 images x 120 alignments of an 8-byte row: 16 alignments per workgroup, the last chunk
# half full (with 17 x 200 a workgroup takes 3 and the last chunk holds 2).
CASES = [(1, 8, 8, 1, 1, 1), (3, 5, 8, 1, 3, 4), (4, 16, 16, 1, 17, 200), (2, 6, 6, 4, 3, 8), (4, 17, 25, 2, 3, 12), (4, 12, 12, 2, 70, 8),
         (4, 64, 64, 4, 3, 8), (4, 64, 64, 1, 2, 648),
         (4, 256, 512, 1, 1, 3), (4, 256, 513, 1, 1, 3), (4, 512, 512, 1, 1, 3), (1, 8, 8, 1, 300, 120)]


@pytest.mark.parametrize("C,H,W,l,B,A", CASES)
def test_rows_align_matches_the_restatement(G, C, H, W, l, B, A):
    codec = G[0]
    rng = np.random.default_rng(C + 3 * H + 7 * W + 11 * l + 13 * B + A)
    rows = rng.integers(0, 256, (B, C * H * W * l // 8), dtype=np.uint8)
    aligns = _align_list(H, W, A)
    assert aligns[0] == (0, 0, 0) and len(aligns) == A
    if A >= 8:
        assert {a[0] for a in aligns} == {d for d in range(8) if H == W or not d & 1}
    want = AR.rows_align(rows, (C, H, W), l, aligns)
    assert np.array_equal(want[:, 0], rows)
    r_dev = torch.from_numpy(rows).cuda()
    table = torch.tensor(aligns, dtype=torch.int32).cuda()
    for name, pattern in (("NAN", NAN), ("FINITE", FINITE)):
        L = Ledger(pattern)
        try:
            with poisoned(L):
                out = codec.rows_align(L.wrap(r_dev), (C, H, W), l, L.wrap(table) if pattern == NAN else aligns)     # a device table, a list
            torch.cuda.synchronize()
            L.check()
            assert L.untouched(out) == _by_chance(want, pattern), f"never written ({name} run) -- {L.where(out)}"
            got = out.cpu().numpy()
        finally:
            L.release()
        assert got.dtype == np.uint8 and got.shape == (B, A, rows.shape[1])
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
        assert np.array_equal(got[:, 0], rows)                                   # the identity row is the input row


def test_every_output_byte_is_written(G):
    """constant rows: all zeros permute to all zeros, which no byte of either pattern (0xFF / 0x7F, 0x4D) equals, so `untouched` must be exactly 0; the bits of
    0xA5 permute to a few distinct bytes, counted exactly.  15- and 425-byte rows start at every address modulo 4."""
    codec = G[0]
    for C, H, W, l, B, A in ((3, 5, 8, 1, 3, 4), (4, 17, 25, 2, 3, 12), (4, 16, 16, 1, 17, 200)):
        aligns = _align_list(H, W, A)
        for fill in (0x00, 0xA5):
            r_dev = torch.full((B, C * H * W * l // 8), fill, dtype=torch.uint8).cuda()
            want = AR.rows_align(r_dev.cpu().numpy(), (C, H, W), l, aligns)
            for pattern in (NAN, FINITE):
                L = Ledger(pattern)
                try:
                    with poisoned(L):
                        out = codec.rows_align(L.wrap(r_dev), (C, H, W), l, aligns)
                    torch.cuda.synchronize()
                    L.check()
                    assert L.untouched(out) == (0 if fill == 0 else _by_chance(want, pattern)), L.where(out)
                    assert np.array_equal(out.cpu().numpy(), want)
                finally:
                    L.release()


@pytest.mark.parametrize("l", [1, 2, 4])
def test_rows_align_is_the_quantiser_of_the_aligned_latent(G, l):
    codec, AL = G[0], G[1]
    z = torch.randn(3, 4, 16, 16, generator=torch.Generator().manual_seed(l)).half().cuda()
    aligns = [(d, 0, 0) for d in range(8)] + [(d, -3, 5) for d in range(8)]
    packed, flags = codec.quant_pack(z, l)
    assert int(flags.abs().sum()) == 0
    out = codec.rows_align(packed, (4, 16, 16), l, aligns)
    for i, a in enumerate(aligns):
        want, _ = codec.quant_pack(AL.apply(z, a).contiguous(), l)
        assert torch.equal(out[:, i], want), (l, a)


def test_rows_align_refuses_before_any_launch(G):
    codec = G[0]
    ok = torch.zeros(2, 8, dtype=torch.uint8).cuda()
    ident = [(0, 0, 0)]
    with pytest.raises(ValueError, match="whole bytes"):
        codec.rows_align(torch.zeros(2, 2, dtype=torch.uint8).cuda(), (1, 3, 3), 1, ident)              # 9 bits
    with pytest.raises(ValueError, match="l must be"):
        codec.rows_align(ok, (1, 8, 8), 3, ident)
    with pytest.raises(ValueError, match="square"):
        codec.rows_align(ok, (1, 4, 16), 1, [(0, 0, 0), (3, 0, 0)])
    with pytest.raises(ValueError, match="0..7"):
        codec.rows_align(ok, (1, 8, 8), 1, [(8, 0, 0)])
    with pytest.raises(ValueError, match="0..7"):
        codec.rows_align(ok, (1, 8, 8), 1, torch.tensor([[0, 0, 0], [-1, 0, 0]], dtype=torch.int32).cuda())
    with pytest.raises(ValueError, match="at least one"):
        codec.rows_align(ok, (1, 8, 8), 1, [])
    with pytest.raises(ValueError, match="HIP device"):
        codec.rows_align(ok.cpu(), (1, 8, 8), 1, ident)
    with pytest.raises(ValueError):
        codec.rows_align(ok, (1, 8, 16), 1, ident)                                                      # rows of 8 bytes, a lattice of 16
    with pytest.raises(ValueError, match="more than"):
        codec.rows_align(ok, (4, 512, 1024), 1, ident)
    with pytest.raises(ValueError):
        codec.rows_align(ok, (1, 8, 8), 1, torch.zeros(1, 3, dtype=torch.int64).cuda())
    with pytest.raises(RuntimeError):
        codec.rows_align(ok, (1, 8, 8), 1, torch.zeros(1, 3, dtype=torch.int32))                        # a host table next to device rows


# ------------------------------------------------------------------------------------------------------------ the search
def _pairs(rng, K):
    return [(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))) for _ in range(K)]


def _key_rows(pairs):
    return torch.from_numpy(np.stack([np.frombuffer(k + n, dtype=np.uint8) for k, n in pairs]).copy()).cuda()


@pytest.fixture(scope="module")
def SEARCH(G):
    """4 x 16 x 16, five images, nine keys of which rows 2 and 6 are the same (key, nonce), 200 alignments; the restatement's statistics, computed once"""
    codec, AL = G[0], G[1]
    rng = np.random.default_rng(419)
    pairs = _pairs(rng, 9)
    pairs[6] = pairs[2]
    z = torch.randn(5, 4, 16, 16, generator=torch.Generator().manual_seed(419)).half()
    aligns = AL.alignments("d4", 2, 16, 16)
    rows = R.sign_rows(z.view(5, -1).double().numpy())
    S = AR.search_stats(rows, (4, 16, 16), 1, aligns, R.keystreams(pairs, 1024), 8)
    return dict(z=z.cuda(), keys=_key_rows(pairs), aligns=aligns, S=S)


@pytest.mark.parametrize("k", [1, 3])
def test_search_keys_matches_the_restatement(G, SEARCH, k):
    AL = G[1]
    S = SEARCH["S"]
    want = AR.merge(S, k)
    assert np.array_equal(S[:, :, 2], S[:, :, 6])                                      # the forced tie: row 6 never comes before row 2
    for order in want[0].tolist():
        assert 6 not in order or (2 in order and order.index(2) < order.index(6))
    assert (want[0] == 6).any() == (k == 3)                                             # (and with three places it does come, right after its twin's stat)
    rowbytes, A = 128, len(SEARCH["aligns"])
    assert A == 200
    for budget, launches in ((None, 1), (2 * A * rowbytes, 3), (70 * rowbytes, 15)):    # one chunk; three chunks of images; the alignments of ONE image cut in three
        calls = []
        real = G[0].key_search_topk
        G[0].key_search_topk = lambda *a, **kw: (calls.append(a[0].shape[0]), real(*a, **kw))[1]
        try:
            got = AL.search_keys(SEARCH["z"], SEARCH["keys"], 8, SEARCH["aligns"], k=k, budget_bytes=budget)
        finally:
            G[0].key_search_topk = real
        assert len(calls) == launches and sum(calls) == 5 * A, (budget, calls)
        for g, w, name in zip(got, want, ("key", "align", "stat")):
            assert g.dtype == torch.int32 and tuple(g.shape) == (5, k)
            assert np.array_equal(g.cpu().numpy(), w), (budget, name, g, w)


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def E2E(G):
    codec, AL, D, T = G
    E = AR.E2E
    pairs, msgs, clean, attacked, z16, blank = AR.e2e_setup()
    ring = D.Keyring()
    for u, (key, nonce) in enumerate(pairs):
        ring.add(f"key-{u}", key, nonce)
    cands = AL.alignments("d4", E["shift"], E["shape"][1], E["shape"][2])
    assert len(cands) == 200
    ks = R.keystreams(pairs, int(np.prod(E["shape"])))
    host = AR.detect_host(z16, cands, ks, E["msg_bytes"], D.log10_p_blind, T.log10_p_any)
    return dict(ring=ring, pairs=pairs, msgs=msgs, clean=clean, attacked=attacked, z16=z16.cuda(), blank=blank, cands=cands, ks=ks, host=host)


def test_detect_latents_sees_through_flips_turns_and_shifts(G, E2E):
    codec, AL, D, T = G
    E = AR.E2E
    limit = math.log10(E["fpr"])
    host = E2E["host"]
    print("log10 p_any with align:", [round(h[3], 1) for h in host])
    # the restatement alone meets the case
    assert [h[0] for h in host] == list(E["rows"]) and all(h[3] <= limit for h in host) and [h[4] for h in host] == E2E["msgs"]
    dev = D.detect_latents(E2E["z16"], E2E["ring"], 8 * E["msg_bytes"], fpr=E["fpr"], align=E2E["cands"])
    for b, (d, h) in enumerate(zip(dev, host)):
        top = d.candidates[0]
        assert d.key_id == f"key-{E['rows'][b]}" == top.key_id and top.index == E["rows"][b]
        assert top.log10_p_any <= limit and (top.index, top.stat, top.log10_p_any) == (h[0], h[2], h[3])
        assert d.alignment == top.alignment == E2E["cands"][h[1]] == AL.inverse(E["attacks"][b], 32, 32)
        restored = AL.apply(torch.from_numpy(E2E["attacked"][b]), d.alignment)
        assert torch.equal(restored, torch.from_numpy(E2E["clean"][b]))                  # exactly the lattice as embedded
        assert d.message == E2E["msgs"][b] and d.flags == 0
        assert D.format_line("x.png", d).endswith(f", alignment: {AL.describe(d.alignment)}")
    # without align only the un-attacked image names its key
    plain = D.detect_latents(E2E["z16"], E2E["ring"], 8 * E["msg_bytes"], fpr=E["fpr"])
    print("log10 p_any without align:", [round(r.candidates[0].log10_p_any, 1) for r in plain])
    assert [r.key_id for r in plain] == [f"key-{E['rows'][0]}"] + [None] * 5
    assert all(r.alignment is None and r.candidates[0].alignment is None and "alignment" not in D.format_line("x.png", r) for r in plain)
    assert plain[0].message == E2E["msgs"][0]
    # k = 3: the runners-up are other keys, each with its own best alignment, none significant
    more = D.detect_latents(E2E["z16"], E2E["ring"], 8 * E["msg_bytes"], k=3, fpr=E["fpr"], align=E2E["cands"])
    for d, one in zip(more, dev):
        assert d.candidates[0] == one.candidates[0] and len({c.index for c in d.candidates}) == 3
        assert all(c.log10_p_any > limit and c.alignment in E2E["cands"] for c in d.candidates[1:])


def test_unwatermarked_latents_name_no_key_with_align(G, E2E):
    codec, AL, D, T = G
    E = AR.E2E
    host = AR.detect_host(E2E["blank"], E2E["cands"], E2E["ks"], E["msg_bytes"], D.log10_p_blind, T.log10_p_any)
    print("blank log10 p_any:", [round(h[3], 2) for h in host])
    assert all(h[3] > math.log10(E["fpr"]) for h in host)                                # the restatement alone meets the case
    dev = D.detect_latents(E2E["blank"].cuda(), E2E["ring"], 8 * E["msg_bytes"], fpr=E["fpr"], align=E2E["cands"])
    for d, h in zip(dev, host):
        top = d.candidates[0]
        assert d.key_id is None and d.message is None and d.alignment is None
        assert (top.index, top.alignment, top.stat, top.log10_p_any) == (h[0], E2E["cands"][h[1]], h[2], h[3])
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        D.detect_latents(E2E["blank"].view(4, -1).cuda(), E2E["ring"], 64, align=E2E["cands"])
    with pytest.raises(ValueError, match="square"):
        D.detect_latents(torch.zeros(1, 4, 16, 32).half().cuda(), E2E["ring"], 64, align=E2E["cands"])


def test_extract_aligned_under_the_known_key(G, E2E):
    codec, AL, D, T = G
    E = AR.E2E
    for b in (1, 4, 5):
        key, nonce = E2E["pairs"][E["rows"][b]]
        r, other = AL.extract_aligned(E2E["z16"][[b, 0]].contiguous(), key, nonce, 8 * E["msg_bytes"], E2E["cands"], fpr=E["fpr"])
        h = E2E["host"][b]
        assert r.alignment == E2E["cands"][h[1]] == AL.inverse(E["attacks"][b], 32, 32) and r.align_index == h[1] and r.stat == h[2]
        assert r.log10_p == T.log10_p_any(D.log10_p_blind(h[2], 64, 64), 200) and r.detected and r.flags == 0
        assert r.bits.tobytes() == E2E["msgs"][b]                                        # all 64 bits
        assert other.detected == (E["rows"][0] == E["rows"][b])                          # image 0 is under another key


def test_extract_reads_under_the_best_alignment(G, E2E):
    """`extract --align`: the batch vote and the single-image vote go through extract_aligned; without the flag the vote is the reference's and reads noise"""
    import types
    from gswm_amd import extract as X
    codec, AL, D, T = G
    E = AR.E2E
    b = 4
    key, nonce = E2E["pairs"][E["rows"][b]]
    bits = "".join(f"{x:08b}" for x in E2E["msgs"][b])
    args = types.SimpleNamespace(key=key, nonce=nonce, message_length=64, l=1, align="d4", align_shift=2)
    out = X.recover_exactracted_message_batch(E2E["z16"][[b, 0]].contiguous(), args)
    assert out[0] == bits and out[0].alignment == AL.inverse(E["attacks"][b], 32, 32)
    assert out[0].log10_p == T.log10_p_any(D.log10_p_blind(E2E["host"][b][2], 64, 64), 200)       # the bound over the A candidates of ONE key
    assert X._alignment_note(out[0]).startswith(f", alignment: {AL.describe(out[0].alignment)}, log10 p, -")
    assert isinstance(out[1], str) and len(out[1]) == 64                      # image 0 is under another key: a string of noise, its alignment whatever scored best
    one = X.recover_exactracted_message(E2E["z16"][b:b + 1], args)
    assert one == bits and one.alignment == out[0].alignment and one.log10_p == out[0].log10_p
    plain = types.SimpleNamespace(key=key, nonce=nonce, message_length=64, l=1)
    assert X.recover_exactracted_message_batch(E2E["z16"][[b]].contiguous(), plain)[0] != bits and X._alignment_note(X.recover_exactracted_message(E2E["z16"][b:b + 1], plain)) == ""


def test_cli_with_align(G, E2E, tmp_path, monkeypatch, capsys):
    """The front end with --align d4 on two generated files.  Synthetic weights are not an autoencoder, so (as in test_gpu_key_search.py) the inversion is
    replaced by latents: the mirrored image and an unwatermarked one, and no model is built.  The rest -- keyring, candidates from the lattice, search,
    detect.txt -- is the real run."""
    from PIL import Image
    from gswm_amd import extract as X
    codec, AL, D, T = G
    E = AR.E2E
    ring_file = tmp_path / "ring.tsv"
    E2E["ring"].save(ring_file)
    d = tmp_path / "imgs"
    d.mkdir()
    rng = np.random.RandomState(5)
    for i in range(2):
        Image.fromarray(rng.randint(0, 256, (64, 64, 3), dtype=np.uint8)).save(str(d / f"img{i}.png"))
    latents = torch.cat([E2E["z16"][1:2], E2E["blank"][:1].cuda()])
    monkeypatch.setattr(X, "invert_decoded_images", lambda arrs, args, **kw: latents[:len(arrs)].clone())
    monkeypatch.setattr(X, "load_models", lambda *a, **kw: None)               # (nothing is inverted: building the synthetic UNet would be most of the test's time)
    D.main(["--images_directory_path", str(d), "--keyring", str(ring_file), "--message_length", "64", "--allow_synthetic_weights", "--num_inference_steps", "2",
            "--width", "256", "--height", "256", "--strict_kernels", "0", "--align", "d4", "--align_shift", "1"])
    out = capsys.readouterr().out
    lines = (d / "detect.txt").read_text().splitlines()
    start = lines.index("=" * 40 + "Batch Start" + "=" * 40)
    info = dict(l.split(",", 1) for l in lines[1:start])
    assert info["align"] == "d4" and info["align_shift"] == "1" and info["keys"] == "12"
    assert lines[start + 1].startswith("SYNTHETIC WEIGHTS,")
    body = lines[start + 2:-1]
    files = X._DirJob(str(d)).files
    assert len(body) == len(files) == 2
    want = D.detect_latents(latents, E2E["ring"], 64, align=AL.alignments("d4", 1, 32, 32))
    for f, line, w in zip(files, body, want):
        assert line == D.format_line(os.path.basename(f), w) and ", alignment: " in line and line in out
    assert body[0].startswith(f"{os.path.basename(files[0])}, key: key-{E['rows'][1]}, log10 p, -") and body[0].endswith(f"message: {E2E['msgs'][1].hex()}, alignment: hflip")
    assert body[1].startswith(f"{os.path.basename(files[1])}, key: none, ") and ", message: none, alignment: " in body[1]
    with pytest.raises(SystemExit):
        D.main(["--images_directory_path", str(d), "--keyring", str(ring_file), "--align_shift", "1"])
