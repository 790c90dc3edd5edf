"""Blind detection, host side: the exact null tail of the blind statistic against brute-force enumeration, the keyring and its files, the front
end's parser, the status codes gsw_key_search_topk returns before any launch, the public surface, and the end-to-end experiments of
tests/test_gpu_key_search.py on the NumPy restatement alone (so that their seeds are known to satisfy them).  No GPU."""
import ctypes
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import gs_oracle as O  # noqa: E402
import key_search_reference as R  # noqa: E402


@pytest.fixture(scope="module")
def D():
    import gswm_amd  # noqa: F401
    from gswm_amd import detect
    return detect


# ------------------------------------------------------------------------------------------------ log10_p_blind
def _brute_law(M, V):
    """the law of sum of M terms |2 Bin(V, 1/2) - V| as exact fractions, by enumeration of the per-term values"""
    term = {}
    for c in range(V + 1):
        a = abs(2 * c - V)
        term[a] = term.get(a, 0) + Fraction(math.comb(V, c), 2 ** V)
    law = {0: Fraction(1)}
    for _ in range(M):
        nxt = {}
        for x, p in law.items():
            for a, q in term.items():
                nxt[x + a] = nxt.get(x + a, 0) + p * q
        law = nxt
    assert sum(law.values()) == 1
    return law


@pytest.mark.parametrize("M,V", [(1, 8), (3, 5), (4, 6), (8, 4)])
def test_log10_p_blind_equals_brute_force_enumeration(D, M, V):
    law = _brute_law(M, V)
    for s in range(M * V + 1):
        p = sum(v for x, v in law.items() if x >= s)
        got = 10.0 ** D.log10_p_blind(s, M, V)
        assert abs(got / float(p) - 1.0) <= 1e-10, (s, got, float(p))


def test_log10_p_blind_at_one_message_bit_is_the_two_sided_soft_tail(D):
    from gswm_amd import trace
    for V in (8, 9, 64):
        for s in range(1, V + 1):
            assert D.log10_p_blind(s, 1, V) == pytest.approx(trace.log10_p_soft(s, V) + math.log10(2.0), abs=1e-12), (V, s)
        assert D.log10_p_blind(0, 1, V) == 0.0


def test_log10_p_blind_over_the_whole_range_of_the_shipped_lattice(D):
    M, V = 256, 64
    vals = [D.log10_p_blind(s, M, V) for s in range(M * V + 1)]
    assert vals[0] == 0.0
    assert vals[-1] == pytest.approx((M - M * V) * math.log10(2.0), rel=1e-12)
    assert all(math.isfinite(v) for v in vals)
    assert all(a >= b for a, b in zip(vals, vals[1:]))
    assert vals[-1] < -4000 and vals[M * V // 2] < -300                    # far below what a float64 probability can hold
    # odd stats are between two points of the support (V even): the tail of the next even one
    assert vals[4001] == vals[4002] and vals[4002] > vals[4003]
    with pytest.raises(ValueError):
        D.log10_p_blind(M * V + 1, M, V)
    with pytest.raises(ValueError):
        D.log10_p_blind(-1, M, V)
    with pytest.raises(ValueError):
        D.log10_p_blind(0, 0, 4)


def test_log10_p_blind_returns_the_chernoff_bound_beyond_65536_bits(D):
    doc = D.log10_p_blind.__doc__
    assert "EXACT" in doc and "CHERNOFF BOUND" in doc and "tilted" in doc
    M, V = 2048, 128                                                        # 262144 bits: a 2048 x 2048 image
    vals = [D.log10_p_blind(s, M, V) for s in range(0, M * V + 1, 997)] + [D.log10_p_blind(M * V, M, V)]
    assert vals[0] == 0.0 and all(math.isfinite(v) for v in vals) and all(a >= b for a, b in zip(vals, vals[1:]))
    assert vals[-1] == pytest.approx((M - M * V) * math.log10(2.0), rel=1e-12)
    # it IS a bound: on a lattice where both exist it lies above the exact tail
    from gswm_amd.detect import _chernoff_log10
    for s in (2000, 2600, 4000, 9000, 16384):
        assert D.log10_p_blind(s, 256, 64) <= _chernoff_log10(s, 256, 64) + 1e-9


# ------------------------------------------------------------------------------------------------ keyring
def _pairs(n, seed=3):
    rs = np.random.RandomState(seed)
    return [(rs.bytes(32), rs.bytes(16)) for _ in range(n)]


def test_keyring_round_trip(D, tmp_path):
    ring = D.Keyring()
    pairs = _pairs(5)
    for i, (k, n) in enumerate(pairs):
        assert ring.add(f"day-{i}", k if i % 2 else k.hex(), n.hex() if i % 3 else n) == i
    assert len(ring) == 5 and ring.key_ids == [f"day-{i}" for i in range(5)] and ring.row_at(3) == pairs[3] and ring.key_at(4) == "day-4"
    rows = ring.packed()
    assert rows.dtype == np.uint8 and rows.shape == (5, 48) and rows.flags["C_CONTIGUOUS"]
    assert all(rows[i].tobytes() == k + n for i, (k, n) in enumerate(pairs))
    path = tmp_path / "ring.tsv"
    ring.save(path)
    assert path.read_text().splitlines()[2] == f"day-2\t{pairs[2][0].hex()}\t{pairs[2][1].hex()}"
    back = D.Keyring.load(path)
    assert back.key_ids == ring.key_ids and np.array_equal(back.packed(), rows)
    assert np.array_equal(D.load_keyring(path).packed(), rows)
    t = ring.to_device("cpu")
    assert t.dtype == torch.uint8 and tuple(t.shape) == (5, 48) and t is ring.to_device("cpu")
    ring.add("later", *pairs[0])                                             # the same pair under another id is a row of its own
    assert ring.packed().shape == (6, 48) and tuple(ring.to_device("cpu").shape) == (6, 48)
    with pytest.raises(ValueError, match="empty"):
        D.Keyring().packed()


def test_keyring_refuses_bad_rows_by_name(D, tmp_path):
    k, n = _pairs(1)[0]
    ring = D.Keyring()
    ring.add("a", k, n)
    with pytest.raises(ValueError, match="already in the keyring"):
        ring.add("a", n + n, n)
    with pytest.raises(ValueError, match="key must be 32 bytes"):
        ring.add("b", k[:31], n)
    with pytest.raises(ValueError, match="nonce must be 16 bytes"):
        ring.add("b", k, n + b"\0")
    with pytest.raises(ValueError, match="hexadecimal"):
        ring.add("b", "zz" * 32, n)
    with pytest.raises(ValueError, match="key id"):
        ring.add("a\tb", k, n)
    with pytest.raises(ValueError, match="key id"):
        ring.add("", k, n)
    with pytest.raises(TypeError):
        ring.add("b", 5, n)
    good = f"{k.hex()}\t{n.hex()}"
    cases = {"cols2": (f"a\t{k.hex()}\n", "expected 'key_id<TAB>key_hex<TAB>nonce_hex'"),
             "cols4": (f"a\t{good}\t00\n", "expected 'key_id<TAB>key_hex<TAB>nonce_hex'"),
             "hex": (f"a\t{k.hex()[:-1]}g\t{n.hex()}\n", "not hexadecimal"),
             "keylen": (f"a\t{k.hex()[:-2]}\t{n.hex()}\n", "key must be 32 bytes"),
             "noncelen": (f"a\t{k.hex()}\t{n.hex()}00\n", "nonce must be 16 bytes"),
             "dup": (f"a\t{good}\n\nb\t{good}\na\t{good}\n", "already in the keyring"),
             "empty": ("\n\n", "no keyring entries")}
    for name, (text, what) in cases.items():
        path = tmp_path / f"{name}.tsv"
        path.write_text(text)
        with pytest.raises(ValueError, match=what) as e:
            D.Keyring.load(path)
        if name != "empty":
            assert f"{path}:{4 if name == 'dup' else 1}:" in str(e.value)


def test_keyring_from_a_gs_insert_log_with_repeated_keys(D, tmp_path):
    from gswm_amd import trace
    pairs = _pairs(3, seed=8)
    log = tmp_path / "info_data.txt"
    order = [0, 1, 0, 2, 1, 0]
    for j, i in enumerate(order):
        O.write_info_data(str(log), pairs[i][0], pairs[i][1], bytes([j]) * 32)
    ring = D.Keyring.from_info_data(log)
    assert ring.key_ids == ["info:1", "info:2", "info:4"] and [ring.row_at(i) for i in range(3)] == pairs
    assert D.load_keyring(log).key_ids == ring.key_ids
    kreg = trace.KeyedRegistry.from_info_data(log)
    assert len(kreg) == 6 and kreg.n_keys == 3
    again = D.Keyring.from_keyed_registry(kreg)
    assert again.key_ids == ring.key_ids and np.array_equal(again.packed(), ring.packed())
    assert np.array_equal(kreg.packed()[[0, 1, 3], :48], ring.packed())       # a packed KeyedRegistry holds the same heads
    with pytest.raises(ValueError, match="empty"):
        D.Keyring.from_keyed_registry(trace.KeyedRegistry(4))


# ------------------------------------------------------------------------------------------------ front end
def test_cli_parser_defaults_and_bounds(D, capsys):
    base = ["--keyring", "ring.tsv"]
    a = D.build_parser().parse_args(base)
    assert (a.message_length, a.fpr, a.top, a.l, a.scheduler, a.num_inference_steps, a.batch_size) == (256, 1e-6, 1, 1, "DDIM", 30, 16)
    assert a.images_directory_path == "" and a.single_image_path == "" and a.model_id == "stabilityai/stable-diffusion-2-1-base"
    a = D.build_parser().parse_args(base + ["--top", "8", "--fpr", "1", "--l", "4", "--message_length", "2048"])
    assert (a.top, a.fpr, a.l, a.message_length) == (8, 1.0, 4, 2048)
    for extra, name in ((["--top", "0"], "--top"), (["--top", "9"], "--top"), (["--fpr", "0"], "--fpr"), (["--fpr", "1.5"], "--fpr"),
                        (["--fpr", "-1e-6"], "--fpr"), (["--l", "3"], "--l"), (["--l", "8"], "--l")):
        with pytest.raises(SystemExit):
            D.build_parser().parse_args(base + extra)
        assert name in capsys.readouterr().err
    with pytest.raises(SystemExit):
        D.build_parser().parse_args([])
    assert "--keyring" in capsys.readouterr().err
    for bad in (0, 12, 2056, -8):
        with pytest.raises(ValueError, match="message_length"):
            D._message_bytes(bad)
    # the existing front ends did not grow a flag
    from gswm_amd import trace, extract
    for parser in (trace.build_parser(), extract.build_parser()):
        assert not [x for x in parser._actions if "--keyring" in x.option_strings]


def test_format_line(D):
    c = [D.KeyCandidate("k7", 7, 9000, -120.5), D.KeyCandidate("k2", 2, 2100, 0.0)]
    assert D.format_line("a.png", D.DetectResult(c, "k7", b"\x01\xff", 0)) == "a.png, key: k7, log10 p, -120.500, message: 01ff, next: k2 (0.000)"
    assert D.format_line("a.png", D.DetectResult(c[1:], None, None, 2)) == "a.png, key: none, log10 p, 0.000, message: none, flags 2"
    assert D.format_line("a.png", ValueError("boom")) == "Error processing a.png: boom"


# ------------------------------------------------------------------------------------------------ status codes that need no device
def test_c_entry_point_refuses_before_any_launch():
    from gswm_amd import _native as N
    lib = N.lib()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(72)                          # never dereferenced: every call below is refused before a launch

    def call(signs=p, B=1, n=256, keys=p, stride=48, mb=4, K=1, k=1, idx=p, stat=p, ws=p):
        return lib.gsw_key_search_topk(signs, B, n, keys, stride, mb, K, k, idx, stat, ws, None)

    bad = [dict(signs=None), dict(keys=None), dict(idx=None), dict(stat=None), dict(ws=None),
           dict(B=0), dict(B=-3), dict(k=0), dict(k=9), dict(k=-1), dict(mb=0), dict(mb=257), dict(mb=-4),
           dict(n=0), dict(n=-256), dict(K=0), dict(K=-1), dict(K=2 ** 31),
           dict(stride=32), dict(stride=47), dict(stride=56), dict(stride=0), dict(stride=-48), dict(keys=odd)]
    for kw in bad:
        assert call(**kw) == N.GSW_ERR_BAD_ARG, kw
    for kw in (dict(n=264), dict(n=8), dict(n=24, mb=2), dict(n=1048576 - 8, mb=256), dict(n=1048576 + 8)):
        assert call(**kw) == N.GSW_ERR_RAGGED, kw
    for kw in (dict(n=1048576 + 256), dict(n=1 << 21), dict(B=65536), dict(n=1 << 21, B=70000)):
        assert call(**kw) == N.GSW_ERR_UNSUPPORTED, kw
    # the order of the classes: a bad argument before a ragged lattice before an unsupported one
    assert call(n=264, k=9) == N.GSW_ERR_BAD_ARG and call(n=(1 << 21) + 8) == N.GSW_ERR_RAGGED
    # workspace_bytes: 0 for what the search refuses, otherwise enough for one list per workgroup and image
    ws = lib.gsw_key_search_workspace_bytes
    for B, K, k in ((0, 5, 1), (-1, 5, 1), (1, 0, 1), (1, -5, 1), (1, 2 ** 31, 1), (1, 5, 0), (1, 5, 9)):
        assert ws(B, K, k) == 0, (B, K, k)
    assert ws(1, 1, 1) == 8 and ws(3, 5, 2) == 3 * 5 * 2 * 8 and ws(2, 2 ** 31 - 1, 8) == ws(2, 100000, 8) > 0
    assert lib.gsw_version() == 500


def test_symbols_are_exported_and_prototyped():
    from gswm_amd import _native as N
    lib = N.lib()
    for name in ("gsw_key_search_workspace_bytes", "gsw_key_search_topk"):
        assert name in N.exported_symbols() and hasattr(lib, name)
    fn = lib.gsw_key_search_topk
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 12
    assert fn.argtypes[2] is ctypes.c_int64 and fn.argtypes[4] is ctypes.c_int64 and fn.argtypes[6] is ctypes.c_int64
    assert lib.gsw_key_search_workspace_bytes.restype is ctypes.c_size_t
    hdr = open(os.path.join(ROOT, "include", "gswm.h")).read()
    assert "int gsw_key_search_topk(" in hdr and "size_t gsw_key_search_workspace_bytes(" in hdr
    import gswm_amd
    assert "detect" in gswm_amd.__all__


def test_python_wrappers_refuse_before_any_launch(D):
    from gswm_amd import codec
    signs, keys = torch.zeros(2, 32, dtype=torch.uint8), torch.zeros(4, 48, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.key_search_topk(signs, 256, keys, 32)
    ring = D.Keyring()
    ring.add("a", bytes(32), bytes(16))
    z = torch.zeros(2, 4, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.detect_latents(z, ring, 8)
    with pytest.raises(ValueError, match="fpr"):
        D.detect_latents(z, ring, 8, fpr=0.0)
    with pytest.raises(ValueError, match="message_length"):
        D.detect_latents(z, ring, 12)
    with pytest.raises(ValueError, match="k must be"):
        D.detect_latents(z, ring, 8, k=9)
    with pytest.raises(ValueError, match="l must be"):
        D.detect_latents(z, ring, 8, l=3)
    with pytest.raises(ValueError, match="empty"):
        D.detect_latents(z, D.Keyring(), 8)
    with pytest.raises(IndexError):
        D.detect_latents(torch.zeros(1, 4, 10, 10), ring, 256)                # 400 lattice bits, 256-bit messages


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_scores_a_planted_codeword_and_its_own_vote():
    """S under the right key is the keyed score of the image's own voted message; a noiseless codeword scores n_bits; under another key the
    statistic stays where the null law puts it"""
    rs = np.random.RandomState(11)
    pairs = _pairs(4, seed=12)
    for n_bits, mb in ((576, 9), (1024, 16), (2048, 4)):
        ks = R.keystreams(pairs, n_bits)
        msg = rs.bytes(mb)
        cw = np.packbits(O.cipher_bits(msg, *pairs[2], n_bits))
        noisy = cw ^ np.packbits((rs.uniform(size=n_bits) < 0.2).astype(np.uint8))
        signs = np.stack([cw, noisy])
        S = R.stats(signs, ks, mb)
        assert S[0, 2] == n_bits and S[0].argmax() == 2 and S[1].argmax() == 2
        assert R.voted_message(cw, ks[2], mb) == msg
        voted = R.voted_message(noisy, ks[2], mb)
        own = np.packbits(O.cipher_bits(voted, *pairs[2], n_bits))
        assert S[1, 2] == n_bits - 2 * int(np.unpackbits(noisy ^ own).sum())   # trace_keyed_topk's score of the voted message
        idx, st = R.topk(S, 8)
        assert idx[:, 0].tolist() == [2, 2] and idx[0, 4:].tolist() == [-1] * 4 and st[0, 4:].tolist() == [R.INT32_MIN] * 4


@pytest.mark.parametrize("sigma", [1.0, 4.0])
def test_end_to_end_experiments_hold_on_the_restatement(D, sigma):
    """tests/test_gpu_key_search.py's end-to-end cases on NumPy-drawn latents with the SAME noise: at sigma 1 the right key and the message, at
    sigma 4 the right key at fpr 1e-6; two unwatermarked images name no key.  (Printed: the bounds this seed gives.)"""
    from gswm_amd import trace
    E = R.E2E
    pairs, msgs, noise, blank = R.e2e_setup()
    n = int(np.prod(E["shape"]))
    ks = R.keystreams(pairs, n)
    z = (torch.from_numpy(R.e2e_host_latents(pairs, msgs)).float() + sigma * noise).half()
    res = R.detect_host(z, ks, E["msg_bytes"], D.log10_p_blind, trace.log10_p_any)
    print(f"sigma {sigma}: log10 p_any {[round(r[2], 1) for r in res]}")
    limit = math.log10(E["fpr"])
    assert [r[0] for r in res] == list(E["rows"]) and all(r[2] <= limit for r in res)
    if sigma == 1.0:
        assert [r[3] for r in res] == msgs
    none = R.detect_host(blank.half(), ks, E["msg_bytes"], D.log10_p_blind, trace.log10_p_any)
    print(f"unwatermarked: log10 p_any {[round(r[2], 2) for r in none]}")
    assert all(r[2] > limit for r in none)
