"""CPU (no GPU): the host side of tracing against records that carry their own keys -- KeyedRegistry and its files, the record rows,
the NumPy oracle keyed_topk_host against a brute force over codewords of the reference-pinned oracle (gs_oracle.cipher_bits), the
identity with the single-key soft score, the argument validation of the new C entry points, the CLI parser."""
import ctypes

import numpy as np
import pytest

from conftest import README_KEY, README_NONCE

import gs_oracle as O
from gswm_amd import _native as N, codec, gs_insert, trace as T

INT32_MIN = -2 ** 31
K1, N1 = bytes.fromhex(README_KEY), bytes.fromhex(README_NONCE)
K2, N2 = bytes(range(32)), bytes(range(16))


def codeword(key, nonce, msg, n):
    return np.packbits(O.cipher_bits(msg, key, nonce, n))


def random_records(rng, U, msg_bytes):
    return [(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8)),
             bytes(rng.integers(0, 256, msg_bytes, dtype=np.uint8))) for _ in range(U)]


# ------------------------------------------------------------------------------------------------------------ registry
def test_keyed_registry_add_and_refuse_by_name():
    r = T.KeyedRegistry()
    assert r.add("alice", K1, N1, "lthero") == 0
    assert r.add("bob", K2.hex(), N2.hex(), "lthero") == 1                   # the same message under another key is another record
    assert r.add("carol", K1, N2, "lthero") == 2                            # ... and under another nonce
    assert r.record("alice") == (K1, N1, codec.pad_message("lthero")) and r.record_at(1) == (K2, N2, codec.pad_message("lthero"))
    assert r.user_ids == ["alice", "bob", "carol"] and r.user_at(2) == "carol" and len(r) == 3
    assert r.n_keys == 3 and r.message_bytes == 32 and r.message_bits == 256
    with pytest.raises(ValueError, match="'alice' is already registered"):
        r.add("alice", K2, N1, "x")
    with pytest.raises(ValueError, match="'dave'.*already registered to 'bob'"):
        r.add("dave", K2, N2, codec.pad_message("lthero"))
    with pytest.raises(ValueError, match="'erin'.*31 bytes"):
        r.add("erin", K1, N1, bytes(31))
    with pytest.raises(ValueError, match="'frank'.*empty"):
        r.add("frank", K1, N1, "")
    with pytest.raises(ValueError, match="'gina'.*key must be 32 bytes"):
        r.add("gina", K1[:31], N1, "x")
    with pytest.raises(ValueError, match="'hal'.*nonce must be 16 bytes"):
        r.add("hal", K1, N1 + b"\0", "x")
    with pytest.raises(ValueError, match="'ivy'.*hexadecimal"):
        r.add("ivy", "zz" * 32, N1, "x")
    for bad in ("tab\tid", "", "line\nbreak", 5):
        with pytest.raises(ValueError, match="user id"):
            r.add(bad, K1, N1, "y")
    with pytest.raises(TypeError):
        r.add("jo", K1, N1, 7)
    assert len(r) == 3
    with pytest.raises(ValueError):
        T.KeyedRegistry(0)
    with pytest.raises(ValueError):
        T.KeyedRegistry(257)
    with pytest.raises(ValueError, match="empty"):
        T.KeyedRegistry().packed()


def test_keyed_registry_save_load_round_trip(tmp_path):
    r = T.KeyedRegistry()
    r.add("alice", K1, N1, "lthero")
    r.add("bob smith", K2, N2, bytes(range(32)))
    p = tmp_path / "keyed.txt"
    r.save(p)
    assert p.read_text() == (f"alice\t{K1.hex()}\t{N1.hex()}\t{codec.pad_message('lthero').hex()}\n"
                             f"bob smith\t{K2.hex()}\t{N2.hex()}\t{bytes(range(32)).hex()}\n")
    q = T.KeyedRegistry.load(p)
    assert q.user_ids == ["alice", "bob smith"] and np.array_equal(q.packed(), r.packed()) and q.message_bits == 256
    assert [q.record_at(i) for i in range(2)] == [r.record_at(i) for i in range(2)]
    assert T.detect_format(p) == "keyed_registry"
    assert T.KeyedRegistry.from_file(p).user_ids == q.user_ids
    bad = tmp_path / "bad.txt"
    bad.write_text(f"alice\t{K1.hex()}\t{N1.hex()}\n")
    with pytest.raises(ValueError, match="bad.txt:1: expected 'user_id<TAB>key_hex<TAB>nonce_hex<TAB>message_hex'"):
        T.KeyedRegistry.load(bad)
    bad.write_text(f"alice\t{K1.hex()}\t{N1.hex()}\tnothex\n")
    with pytest.raises(ValueError, match="'alice' is not hexadecimal"):
        T.KeyedRegistry.load(bad)
    bad.write_text("\n")
    with pytest.raises(ValueError, match="no registry entries"):
        T.KeyedRegistry.load(bad)


def _write_log(log):
    m = [codec.pad_message(s) for s in ("one", "two", "three")]
    gs_insert._write_info(log, K1, N1, m[0])
    gs_insert._write_info(log, K2, N2, m[1])
    gs_insert._write_info(log, K1, N1, m[2], extra=["use_seed: 1"])
    gs_insert._write_info(log, K1, N1, m[0])                                  # record 1 issued again: dropped
    gs_insert._write_info(log, K1, N2, m[1])                                  # message of record 2 under another key: kept
    return m


def test_keyed_registry_from_info_data_keeps_every_key(tmp_path):
    log = tmp_path / "info_data.txt"
    m = _write_log(log)
    r = T.KeyedRegistry.from_info_data(log)
    assert r.user_ids == ["info:1", "info:2", "info:3", "info:5"]
    assert [r.record(u) for u in r.user_ids] == [(K1, N1, m[0]), (K2, N2, m[1]), (K1, N1, m[2]), (K1, N2, m[1])]
    assert r.n_keys == 3
    # the numbering is Registry.from_info_data's
    assert T.Registry.from_info_data(log, key=K1, nonce=N1).user_ids == ["info:1", "info:3"]
    assert T.Registry.from_info_data(log, key=K1, nonce=N2).user_ids == ["info:5"]
    assert T.KeyedRegistry.from_file(log).user_ids == r.user_ids
    empty = tmp_path / "empty_log.txt"
    empty.write_text("Time: now\n----------------------\n")
    with pytest.raises(ValueError, match="no records"):
        T.KeyedRegistry.from_info_data(empty)


def test_formats_are_told_apart(tmp_path):
    log, two, four = tmp_path / "info_data.txt", tmp_path / "two.txt", tmp_path / "four.txt"
    _write_log(log)
    single = T.Registry()
    single.add("alice", "lthero")
    single.save(two)
    keyed = T.KeyedRegistry()
    keyed.add("alice", K1, N1, "lthero")
    keyed.save(four)
    assert (T.detect_format(log), T.detect_format(two), T.detect_format(four)) == ("info_data", "registry", "keyed_registry")
    assert T.Registry.from_file(two).user_ids == ["alice"] and T.Registry.from_file(log, K2, N2).user_ids == ["info:2"]
    with pytest.raises(ValueError, match="single-key registry"):
        T.KeyedRegistry.from_file(two)
    # a four-column file is not a registry of 80-byte messages
    with pytest.raises(ValueError, match="four.txt:1: expected 'user_id<TAB>message_hex'"):
        T.Registry.load(four)
    with pytest.raises(ValueError, match="expected 'user_id<TAB>message_hex'"):
        T.Registry.from_file(four)


@pytest.mark.parametrize("msg_bytes,stride", [(1, 64), (5, 64), (16, 64), (17, 80), (32, 80), (128, 176), (256, 304)])
def test_packed_rows_are_key_nonce_message_at_the_documented_stride(msg_bytes, stride):
    rng = np.random.default_rng(msg_bytes)
    recs = random_records(rng, 7, msg_bytes)
    r = T.KeyedRegistry(msg_bytes)
    for i, (k, n, m) in enumerate(recs):
        r.add(f"u{i}", k, n, m)
    rows = r.packed()
    assert rows.dtype == np.uint8 and rows.shape == (7, stride) and rows.flags["C_CONTIGUOUS"]
    assert r.record_stride == stride == codec.keyed_record_stride(msg_bytes) and stride % 16 == 0 and stride >= 48 + msg_bytes
    for i, (k, n, m) in enumerate(recs):
        assert rows[i, :32].tobytes() == k and rows[i, 32:48].tobytes() == n and rows[i, 48:48 + msg_bytes].tobytes() == m
        assert not rows[i, 48 + msg_bytes:].any()
    assert r.packed() is rows                                                 # cached
    r.add("late", K1, N1, bytes(msg_bytes))
    assert r.packed().shape == (8, stride)                                    # ... until the registry changes


# ------------------------------------------------------------------------------------------------------------ top-k oracle
def brute_force(signs, records, n, k):
    """Python integers, explicit bit extraction (bit i -> byte i >> 3, bit 7 - (i & 7)), codewords from the oracle's cipher_bits"""
    out_idx, out_score = [], []
    cw = [O.cipher_bits(m, key, nonce, n) for key, nonce, m in records]
    for row in signs:
        scored = []
        for u, e in enumerate(cw):
            d = sum(((int(row[i >> 3]) >> (7 - (i & 7))) & 1) ^ int(e[i]) for i in range(n))
            scored.append((-(n - 2 * d), u))
        scored.sort()
        scored = scored[:k]
        out_idx.append([u for _, u in scored] + [-1] * (k - len(scored)))
        out_score.append([-s for s, _ in scored] + [INT32_MIN] * (k - len(scored)))
    return np.array(out_idx, dtype=np.int32), np.array(out_score, dtype=np.int32)


@pytest.mark.parametrize("U,n,msg_bytes,B,k", [(5, 64, 4, 3, 2), (9, 8, 1, 2, 8), (3, 520, 5, 4, 4), (17, 1024, 32, 2, 3), (1, 16, 2, 1, 1)])
def test_keyed_topk_host_matches_brute_force(U, n, msg_bytes, B, k):
    rng = np.random.default_rng(U * 100 + n + B)
    recs = random_records(rng, U, msg_bytes)
    signs = rng.integers(0, 256, (B, n // 8), dtype=np.uint8)
    cw = np.stack([codeword(key, nonce, m, n) for key, nonce, m in recs])
    idx, score = T.keyed_topk_host(signs, cw, k)
    want_idx, want_score = brute_force(signs, recs, n, k)
    assert idx.dtype == np.int32 and score.dtype == np.int32
    assert np.array_equal(idx, want_idx) and np.array_equal(score, want_score)


def test_keyed_topk_host_ties_go_to_the_lower_index_and_pads_past_the_registry():
    n = 64
    recs = [(K2, N2, b"\x01" * 4), (K1, N1, b"abcd"), (K1, N1, b"abcd"), (K2, N1, b"wxyz"), (K1, N1, b"abcd")]    # rows 1, 2, 4: one codeword
    cw = np.stack([codeword(key, nonce, m, n) for key, nonce, m in recs])
    signs = cw[1:2].copy()
    signs[0, 3] ^= 0x10                                                      # one differing bit
    idx, score = T.keyed_topk_host(signs, cw, 8)
    assert idx[0, :3].tolist() == [1, 2, 4] and score[0, :3].tolist() == [n - 2] * 3
    assert idx[0, 5:].tolist() == [-1] * 3 and score[0, 5:].tolist() == [INT32_MIN] * 3
    bi, bs = brute_force(signs, recs, n, 8)
    assert np.array_equal(idx, bi) and np.array_equal(score, bs)
    with pytest.raises(ValueError):
        T.keyed_topk_host(signs, cw[:, :4], 1)


@pytest.mark.parametrize("n,M", [(256, 8), (520, 40), (1024, 256), (16384, 256), (16384, 1024), (4608, 64)])
def test_shared_key_scores_are_the_soft_scores(n, M):
    """For records that share one key, n - 2 popcount(h ^ e) is the soft score sum_t (2 r - 1)(2 c - V) on the vote counts"""
    rng = np.random.default_rng(n + M)
    U, B, V = 40, 5, n // M
    msgs = rng.integers(0, 256, (U, M // 8), dtype=np.uint8)
    z = rng.standard_normal((B, n))
    z[0] = np.abs(z[0])                                                       # all sign bits 1
    z[1] = -np.abs(z[1])                                                      # all sign bits 0
    h = np.stack([np.packbits(O.quantise(z[b]).astype(np.uint8)) for b in range(B)])
    ks = np.unpackbits(np.frombuffer(O.chacha20_keystream(K1, N1, n // 8), dtype=np.uint8))
    counts = np.stack([(np.unpackbits(h[b]) ^ ks).reshape(V, M).sum(axis=0) for b in range(B)])      # the reference's vote, extract.py:88-99
    cw = np.stack([codeword(K1, N1, msgs[u].tobytes(), n) for u in range(U)])
    for k in (1, 8):
        a = T.keyed_topk_host(h, cw, k)
        b = T.topk_host(counts, V, msgs, k, True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_keyed_entry_points_validate_before_any_hip_call():
    lib, p = N.lib(), ctypes.c_void_p(16)
    BAD, UNS, RAG = N.GSW_ERR_BAD_ARG, N.GSW_ERR_UNSUPPORTED, N.GSW_ERR_RAGGED

    def call(signs=p, B=2, n=16384, rec=p, stride=80, mb=32, U=100, k=4, idx=p, score=p, ws=p):
        return lib.gsw_trace_keyed_topk(signs, B, n, rec, stride, mb, U, k, idx, score, ws, None)

    for name in ("signs", "rec", "idx", "score", "ws"):
        assert call(**{name: None}) == BAD, name
    assert call(B=0) == BAD and call(B=-1) == BAD
    assert call(k=0) == BAD and call(k=9) == BAD
    assert call(mb=0) == BAD and call(mb=257, stride=320) == BAD and call(mb=-4) == BAD
    assert call(U=0) == BAD and call(U=-5) == BAD and call(U=2 ** 31) == BAD
    for stride in (79, 64, 72, 88, 0, -80):                                   # too short for key | nonce | message, or not a multiple of 16
        assert call(stride=stride) == BAD, stride
    assert call(rec=ctypes.c_void_p(8)) == BAD                                # rows are read as aligned dwords
    assert call(n=0) == BAD and call(n=-256) == BAD
    for n in (16384 + 8, 250, 255, 16384 + 128):                              # not a multiple of 8 msg_bytes
        assert call(n=n) == RAG, n
    assert call(n=48, mb=5, stride=64) == RAG and call(n=8, mb=5, stride=64) == RAG
    assert call(n=2 ** 20 + 256) == UNS and call(n=2 ** 40) == UNS and call(B=65536) == UNS
    assert call(mb=256, stride=304, n=2048 * 7 + 8) == RAG
    assert lib.gsw_version() == 500

    def pack(z=p, dt=N.GSW_F16, signs=p, flags=p, B=2, n=16384):
        return lib.gsw_sign_pack(z, dt, signs, flags, B, n, None)

    for name in ("z", "signs", "flags"):
        assert pack(**{name: None}) == BAD, name
    assert pack(dt=4) == BAD and pack(dt=-1) == BAD and pack(B=-1) == BAD and pack(n=0) == BAD and pack(n=-8) == BAD
    assert pack(n=16383) == UNS and pack(n=4) == UNS and pack(n=2 ** 31) == UNS
    assert pack(B=0) == N.GSW_OK                                              # nothing to do, as gsw_extract


def test_keyed_workspace_is_monotone():
    f = N.lib().gsw_trace_keyed_workspace_bytes
    assert f(1, 1, 1) > 0
    Bs, Us, ks = (1, 3, 16, 17, 64, 130, 1000), (1, 63, 256, 257, 4097, 2 ** 17 + 3, 2 ** 24, 2 ** 31 - 1), (1, 2, 4, 8)
    for U in Us:
        for k in ks:
            v = [f(B, U, k) for B in Bs]
            assert v == sorted(v) and v[0] > 0 and len(set(v)) == len(v)
    for B in Bs:
        for k in ks:
            v = [f(B, U, k) for U in Us]
            assert v == sorted(v)
        for U in Us:
            v = [f(B, U, k) for k in ks]
            assert v == sorted(v) and len(set(v)) == len(v)
    assert f(0, 10, 1) == 0 and f(1, 0, 1) == 0 and f(1, 10, 9) == 0 and f(1, 10, 0) == 0 and f(1, 2 ** 31, 1) == 0
    assert f(64, 2 ** 24, 8) <= 4 << 20                                       # partial lists, not scores


def test_keyed_wrappers_have_no_cpu_path():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.sign_pack(torch.zeros(1, 4, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.trace_keyed_topk(torch.zeros(1, 32, dtype=torch.uint8), 256, torch.zeros(4, 80, dtype=torch.uint8), 32)


# ------------------------------------------------------------------------------------------------------------ CLI
def test_cli_parser_per_record_keys():
    P = T.build_parser()
    old = P.parse_args(["--key_hex", README_KEY, "--nonce_hex", "", "--registry", "r.txt", "--hard", "--top", "3"])
    assert (old.key_hex, old.nonce_hex, old.registry, old.hard, old.top, old.per_record_keys) == (README_KEY, "", "r.txt", True, 3, False)
    a = P.parse_args(["--per_record_keys", "--registry", "info_data.txt", "--fpr", "1e-9", "--top", "2"])
    assert a.per_record_keys is True and a.key_hex is None and a.nonce_hex is None and (a.fpr, a.top, a.hard) == (1e-9, 2, False)
    for bad in (["--registry", "r.txt"],                                                       # no key and no --per_record_keys: as before
                ["--key_hex", README_KEY, "--registry", "r.txt"], ["--nonce_hex", "", "--registry", "r.txt"],
                ["--per_record_keys", "--registry", "r.txt", "--hard"],
                ["--per_record_keys", "--registry", "r.txt", "--key_hex", README_KEY],
                ["--per_record_keys"]):
        with pytest.raises(SystemExit):
            P.parse_args(bad)
    assert "--per_record_keys" in P.format_help()


def test_cli_refuses_hard_with_per_record_keys_by_name(capsys):
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--per_record_keys", "--registry", "r.txt", "--hard"])
    err = capsys.readouterr().err
    assert "--hard" in err and "--per_record_keys" in err and "soft" in err
