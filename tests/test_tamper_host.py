"""CPU (no GPU): the host side of the tamper map and the tile-weighted vote -- the exact tile threshold against scipy, the default weights, the
NumPy restatement (tests/tamper_reference.py) against the oracle's vote and its gain on damaged synthetic latents, the map's verdicts against the
ground truth, and that trace / extract are what they were when the new flags are off."""
import numpy as np
import pytest

from conftest import README_KEY, README_NONCE

import gs_oracle as O
import tamper_reference as R

import gswm_amd  # noqa: F401
from gswm_amd import codec, extract as X, tamper, trace as T

KEY, NONCE = bytes.fromhex(README_KEY), bytes.fromhex(README_NONCE)
SHAPE, M, TILE, N_T = (4, 64, 64), 256, 8, 256
NB = 4 * 64 * 64
MSG = bytes(np.random.default_rng(77).integers(0, 256, 32, dtype=np.uint8))
SEEDS, IMAGES, REPLACED = (0, 1, 2), 20, 48


# ------------------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("n_t", [256, 1024, 4096, 16384])
@pytest.mark.parametrize("fpr", [1e-3, 1e-6, 1e-12])
def test_tile_threshold_is_scipys_isf(n_t, fpr):
    """isf(q) is the smallest x with P[X > x] <= q, so the smallest k with P[X >= k] <= q is isf(q) + 1.  Exact, no tolerance."""
    from scipy.stats import binom
    for n_tiles in (1, 64):
        k = tamper.tile_threshold(n_t, n_tiles, fpr)
        assert k == int(binom.isf(fpr / n_tiles, n_t, 0.5)) + 1
        bound = fpr / n_tiles
        assert T._binomial_tail(n_t, k) / (1 << n_t) <= bound < T._binomial_tail(n_t, k - 1) / (1 << n_t)


def test_tile_threshold_edges():
    assert tamper.tile_threshold(8, 1, 1.0) == 0                         # every count is as likely as that
    assert tamper.tile_threshold(8, 1, 2.0 ** -8) == 8                   # only agree == n_t is that rare
    assert tamper.tile_threshold(8, 2, 2.0 ** -8) == 9                   # not even that: no count proves anything
    for bad in ((0, 1, 0.5), (8, 0, 0.5), (8, 1, 0.0), (8, 1, 1.5)):
        with pytest.raises(ValueError):
            tamper.tile_threshold(*bad)


def test_default_weights_clamp_and_top():
    import torch
    slack = 16                                                            # isqrt(256)
    a = np.array([[0, 128, 136], [137, 200, 256]])
    want = np.array([[0, 0, 0], [2, 128, 240]], dtype=np.uint16)          # 2 a - 256 - 16, clamped at 0; agree == n_t -> n_t - slack
    got = tamper.default_weights(a, 256)
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    t = tamper.default_weights(torch.from_numpy(a.astype(np.int32)), 256)
    assert t.dtype == torch.uint16 and np.array_equal(t.view(torch.int16).numpy().astype(np.uint16), want)
    assert tamper.weight_slack(256) == slack and tamper.weight_slack(16384) == 128
    assert int(tamper.default_weights([16384], 16384)[0]) == 16384 - 128  # the largest weight there is fits uint16
    assert np.array_equal(R.default_weights(a, 256), want)
    with pytest.raises(ValueError):
        tamper.default_weights(a, 16385)


# ------------------------------------------------------------------------------------------------------------ the restatement
def _accuracy(bits):
    return float((np.asarray(bits) == np.unpackbits(np.frombuffer(MSG, dtype=np.uint8))).mean())


def test_restatement_with_unit_weights_is_the_oracles_vote():
    z = R.synthetic_latents(MSG, KEY, NONCE, SHAPE, 1.0, 5, 2, replaced_rows=REPLACED)
    ks = O.keystream_bits(KEY, NONCE, NB)
    for b in range(2):
        bits, score, wsum = R.vote(R.quantise_bits(z[b]), ks, np.ones((8, 8)), M, SHAPE, 1, TILE)
        assert "".join(map(str, bits)) == O.recover_bits(z[b], KEY, NONCE, M)
        assert np.all(wsum == 64) and np.all(np.abs(score) <= 64)
        r0 = R.robust(R.quantise_bits(z[b]), KEY, NONCE, M, SHAPE, 1, TILE, iters=0)
        assert np.array_equal(r0[0], bits)
    # l = 2: the map's tiles partition the row and a codeword agrees with itself everywhere
    cw = R.codeword(MSG, KEY, NONCE, 2 * NB)
    assert np.array_equal(R.tile_agree(cw, cw, SHAPE, 2, 16), np.full((4, 4), 4 * 16 * 16 * 2))


@pytest.fixture(scope="module")
def damaged_runs():
    """per sigma/damage: [(plain accuracy, weighted accuracy)] over SEEDS x IMAGES synthetic latents, computed once"""
    def run(sigma, replaced):
        out = []
        for seed in SEEDS:
            z = R.synthetic_latents(MSG, KEY, NONCE, SHAPE, sigma, seed, IMAGES, replaced_rows=replaced)
            for b in range(IMAGES):
                q = R.quantise_bits(z[b])
                out.append((_accuracy(R.robust(q, KEY, NONCE, M, SHAPE, 1, TILE, iters=0)[0]), _accuracy(R.robust(q, KEY, NONCE, M, SHAPE, 1, TILE, iters=2)[0])))
        return np.array(out)
    return {"damaged": run(1.0, REPLACED), "clean": run(1.5, 0)}


def test_weighted_vote_gains_on_damaged_latents(damaged_runs):
    plain, weighted = damaged_runs["damaged"].mean(axis=0)
    print(f"sigma 1.0, 48 of 64 rows replaced: plain {plain:.4f}, weighted {weighted:.4f}")
    assert weighted >= plain + 0.05


def test_weighted_vote_costs_nothing_on_intact_latents(damaged_runs):
    plain, weighted = damaged_runs["clean"].mean(axis=0)
    print(f"sigma 1.5, nothing replaced: plain {plain:.4f}, weighted {weighted:.4f}")
    assert weighted >= plain - 0.002


def test_known_message_map_is_the_ground_truth():
    """sigma = 0.5, the top 48 rows replaced, fpr = 1e-6, tile 8: `intact` must be exactly the two bottom tile rows on every one of the 60 images"""
    cw = R.codeword(MSG, KEY, NONCE, NB)
    truth = np.zeros((8, 8), dtype=bool)
    truth[REPLACED // TILE:] = True
    thr = tamper.tile_threshold(N_T, 64, 1e-6)
    assert 170 <= thr <= 176
    weakest, strongest = N_T, 0
    for seed in SEEDS:
        z = R.synthetic_latents(MSG, KEY, NONCE, SHAPE, 0.5, seed, IMAGES, replaced_rows=REPLACED)
        for b in range(IMAGES):
            tm = tamper.make_map(R.tile_agree(R.quantise_bits(z[b]), cw, SHAPE, 1, TILE), N_T, TILE, 1e-6, "message")
            weakest, strongest = min(weakest, int(tm.agree[truth].min())), max(strongest, int(tm.agree[~truth].max()))
            assert np.array_equal(tm.intact, truth), (seed, b)
            assert tm.log10_p is not None and tm.log10_p.shape == (8, 8) and (tm.log10_p[truth] < -6 - np.log10(64)).all()
    print(f"weakest intact tile {weakest}/256, strongest replaced tile {strongest}/256, threshold {thr}")
    assert strongest < thr <= weakest


def test_make_map_labels():
    a = np.array([[256, 128], [180, 100]])
    tm = tamper.make_map(a, 256, 8, 1e-6, "decoded")
    assert tm.log10_p is None and tm.source == "decoded" and tm.agree.dtype == np.int32 and tm.n_intact == 2 and tm.n_tiles == 4
    tm = tamper.make_map(a, 256, 8, 1e-6, "registry")
    assert tm.log10_p[0, 0] == T.log10_p_soft(256, 256) == -256 * np.log10(2.0) and tm.log10_p[0, 1] == T.log10_p_soft(0, 256)
    with pytest.raises(ValueError):
        tamper.make_map(a, 256, 8, 1e-6, "guess")


def test_save_map_writes_counts_and_picture(tmp_path):
    from PIL import Image
    a = np.array([[256, 128, 200], [180, 100, 90]])
    tm = tamper.make_map(a, 256, 8, 1e-6, "message")
    npy, png = tamper.save_map(tm, str(tmp_path / "maps" / "img0"), (192, 128))
    assert npy.endswith("img0.tamper.npy") and png.endswith("img0.tamper.png")
    back = np.load(npy)
    assert back.dtype == np.int32 and np.array_equal(back, a)
    im = Image.open(png)
    assert im.mode == "L" and im.size == (192, 128)                       # 3 x 2 tiles of 8 x 8 lattice elements of 8 x 8 pixels
    px = np.asarray(im)
    assert np.array_equal(px[32::64, 32::64], np.where(tm.intact, 255, 0)) and set(np.unique(px)) <= {0, 255}
    assert tamper.map_stem("out", "/a/b/cat.jpg") == "out/cat"


# ------------------------------------------------------------------------------------------------------------ nothing else changed
def test_trace_result_and_format_line_are_unchanged_without_a_map():
    r = T.TraceResult()
    assert r.candidates == [] and r.attributed is None and r.tamper is None
    r = T.TraceResult([T.Candidate("u1", 1, 900, 250, -30.5), T.Candidate("u2", 2, 10, 130, 0.0)], "u1")
    line = "a.png, user: u1, agreement, 0.9765625, log10 p, -30.500, next: u2 (0.5078125, 0.000)"
    assert T.format_line("a.png", r, 256) == line
    r.tamper = tamper.make_map(np.array([[256, 128]]), 256, 8, 1e-6, "registry")
    assert T.format_line("a.png", r, 256) == line + ", intact tiles 1/2"
    assert T.format_line("a.png", T.TraceResult(), 256) == "a.png, user: none, agreement, nan, log10 p, 0.0"
    assert T.format_line("a.png", ValueError("boom"), 256) == "Error processing a.png: boom"


def test_cli_parsers_accept_the_new_flags_and_keep_their_defaults():
    base = ["--key_hex", README_KEY, "--nonce_hex", README_NONCE]
    a = T.build_parser().parse_args(base + ["--registry", "r.txt"])
    assert a.tamper_map is None and a.tile == 8 and a.top == 1 and a.fpr == 1e-6 and a.l == 1 and a.batch_size == 16
    a = T.build_parser().parse_args(base + ["--registry", "r.txt", "--tamper_map", "out", "--tile", "32"])
    assert a.tamper_map == "out" and a.tile == 32
    x = X.build_parser().parse_args(base + ["--original_message_hex", "00"])
    assert x.robust == 0 and x.tamper_map is None and x.tile == 8 and x.message_length == 1024 and x.l == 1 and x.batch_size == 16
    x = X.build_parser().parse_args(base + ["--original_message_hex", "00", "--robust", "1", "--tamper_map", "out", "--tile", "16"])
    assert x.robust == 1 and x.tamper_map == "out" and x.tile == 16
    for parser, extra in ((T.build_parser(), ["--registry", "r.txt"]), (X.build_parser(), ["--original_message_hex", "00"])):
        with pytest.raises(SystemExit):
            parser.parse_args(base + extra + ["--tile", "4"])


def test_wrappers_refuse_before_touching_a_device():
    import torch
    p, k = torch.zeros(2, 128, dtype=torch.uint8), torch.zeros(2, 48, dtype=torch.uint8)
    with pytest.raises(ValueError, match="tile must be one of"):
        codec.tile_agreement(p, k, torch.zeros(2, 8, dtype=torch.uint8), 64, (4, 16, 16), 1, 4)
    with pytest.raises(ValueError, match="whole number"):
        codec.vote_tiled(p, k, torch.zeros(2, 1, 1, dtype=torch.int16).view(torch.uint16), 64, (4, 16, 20), 1, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.tile_agreement(p, k, torch.zeros(2, 8, dtype=torch.uint8), 64, (4, 16, 16), 1, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.vote_tiled(p, k, torch.ones(2, 2, 2, dtype=torch.int16).view(torch.uint16), 64, (4, 16, 16), 1, 8)
