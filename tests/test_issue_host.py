"""Host side of issuing (gswm_amd/issue.py): requests, the checks made before any device call, the info_data.txt text, the command line.  No GPU."""
import ast
import os
import re

import numpy as np
import pytest

import gswm_amd  # noqa: F401
from gswm_amd import codec, issue
from gswm_amd.gs_insert import _write_info
from gswm_amd.trace import KeyedRegistry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY, NONCE = "5822ff9cce6772f714192f43863f6bad1bf54b78326973897e6b66c3186b77a7", "05072fd1c2265f6f2e2a4080a2bfbdd8"


# ---------------------------------------------------------------------------------------------------------------- Request
def test_request_str_and_bytes_messages():
    r = issue.Request("alice", "lthero", KEY, NONCE)
    assert r.record(32) == (bytes.fromhex(KEY), bytes.fromhex(NONCE), codec.pad_message("lthero", 32))
    assert r.record(4)[2] == b"lthe"                                                # truncated as gs_insert truncates
    b = issue.Request("bob", bytes(range(32)), bytes.fromhex(KEY), bytes.fromhex(NONCE))          # key and nonce as bytes
    assert b.record(32) == (bytes.fromhex(KEY), bytes.fromhex(NONCE), bytes(range(32)))
    with pytest.raises(ValueError, match="'bob'.*32 bytes.*16-byte"):
        b.record(16)
    with pytest.raises(ValueError, match="'carol'.*empty message"):
        issue.Request("carol", "")
    with pytest.raises(TypeError, match="'carol'"):
        issue.Request("carol", 7)
    with pytest.raises(ValueError):
        issue.Request("two\tcolumns", "x")


def test_blank_keys_are_drawn_per_request():
    a, b = issue.Request("alice", "same message"), issue.Request("bob", "same message")
    assert len(a.key) == 32 and len(a.nonce) == 16 and len(b.key) == 32 and len(b.nonce) == 16
    assert a.key != b.key and a.nonce != b.nonce
    assert a.record(32) == a.record(32)                                             # drawn once, at construction
    k = issue.Request("carol", "x", KEY)                                            # key only: gs_insert.py:33-36
    assert k.key == bytes.fromhex(KEY) and k.nonce == bytes.fromhex(KEY[16:48])
    assert issue.Request("dave", "x", "", "").key != issue.Request("dave", "x", None, None).key


@pytest.mark.parametrize("key,nonce,what", [("zz" * 32, NONCE, "hexadecimal"), (KEY[:-2], NONCE, "key must be 32 bytes"), (KEY, NONCE + "00", "nonce must be 16 bytes"),
                                            (KEY, "xy", "hexadecimal"), (None, NONCE, "nonce without a key"), (b"\x00" * 31, None, "key must be 32 bytes")])
def test_bad_key_or_nonce_is_refused_by_name(key, nonce, what):
    with pytest.raises(ValueError, match=f"'mallory'.*{what}"):
        issue.Request("mallory", "x", key, nonce)


# ---------------------------------------------------------------------------------------------------------------- checks before the device
def _registry():
    reg = KeyedRegistry(32)
    reg.add("alice", KEY, NONCE, "alice@example")
    return reg


def test_clashes_are_raised_before_any_device_call(monkeypatch):
    reg = _registry()

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(codec, "embed_records", no_device)
    monkeypatch.setattr(codec, "mt19937_uniform", no_device)
    # a user id already bound to another triple
    with pytest.raises(ValueError, match="'alice' is already bound"):
        issue.issue_latents([issue.Request("bob", "bob"), issue.Request("alice", "another message", KEY, NONCE)], registry=reg)
    # a triple already bound to another user
    with pytest.raises(ValueError, match="'eve'.*already bound to 'alice'"):
        issue.issue_latents([issue.Request("eve", "alice@example", KEY, NONCE)], registry=reg)
    # among the requests themselves
    with pytest.raises(ValueError, match="'bob' is already bound"):
        issue.issue_latents([issue.Request("bob", "one"), issue.Request("bob", "two")], registry=reg)
    with pytest.raises(ValueError, match="'eve'.*already bound to 'bob'"):
        issue.issue_latents([issue.Request("bob", "m", KEY, NONCE), issue.Request("eve", "m", KEY, NONCE)])
    with pytest.raises(ValueError, match="'bob'.*16 bytes"):
        issue.issue_latents([issue.Request("bob", b"\x00" * 16)], registry=reg)
    with pytest.raises(ValueError, match="no requests"):
        issue.issue_latents([], registry=reg)
    with pytest.raises(ValueError):
        issue.issue_latents([issue.Request("bob", "bob")], registry=reg, l=3)
    assert reg.user_ids == ["alice"]                                                # nothing was added on the way


def test_resolve_requests_accepts_a_repeat_and_changes_nothing():
    reg = _registry()
    reqs = [issue.Request("alice", "alice@example", KEY, NONCE), issue.Request("bob", "bob"), issue.Request("bob", "bob")]
    reqs[2].key, reqs[2].nonce = reqs[1].key, reqs[1].nonce                         # the same user twice under one record: two images of one watermark
    recs = issue.resolve_requests(reqs, reg)
    assert recs[0] == reg.record("alice") and recs[1] == recs[2] and len(reg) == 1
    rows = issue.pack_records(recs, 32)
    assert rows.shape == (3, 80) and rows.dtype == np.uint8
    assert bytes(rows[1, :32]) == reqs[1].key and bytes(rows[1, 32:48]) == reqs[1].nonce and bytes(rows[1, 48:]) == codec.pad_message("bob", 32)
    reg.add("bob", *recs[1])
    assert np.array_equal(rows[:2], reg.packed())                                   # KeyedRegistry.packed's row format
    assert issue.pack_records(issue.resolve_requests([issue.Request("x", b"\x07" * 5)], None, 5), 5).shape == (1, 64)


# ---------------------------------------------------------------------------------------------------------------- the log
def test_log_text_is_write_infos_and_reads_back(tmp_path):
    reqs = [issue.Request("alice", "alice@example"), issue.Request("bob", bytes(range(32)), KEY, NONCE), issue.Request("carol", "carol", KEY)]
    recs = issue.resolve_requests(reqs)
    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    issue.write_log(a, recs)
    for rec in recs:
        _write_info(b, *rec)
    strip = lambda p: re.sub(r"^Time: .*$", "Time:", open(p).read(), flags=re.M)    # noqa: E731
    assert strip(a) == strip(b) and open(a).read().count("----------------------\n") == 3
    back = KeyedRegistry.from_info_data(a)
    assert [back.record_at(i) for i in range(len(back))] == recs
    assert back.user_ids == ["info:1", "info:2", "info:3"]


# ---------------------------------------------------------------------------------------------------------------- command line
def test_parser_defaults_and_choices():
    p = issue.build_parser()
    a = p.parse_args(["--requests", "r.tsv", "--registry", "reg.tsv"])
    assert (a.height, a.width, a.l, a.seed, a.dtype, a.info_data, a.out_dir, a.fast) == (512, 512, 1, None, "float32", None, None, False)
    a = p.parse_args(["--requests", "r.tsv", "--registry", "reg.tsv", "--info_data", "i.txt", "--out_dir", "d", "--height", "768", "--width", "1024", "--l", "4",
                      "--seed", "9", "--dtype", "float16"])
    assert (a.height, a.width, a.l, a.seed, a.dtype, a.info_data, a.out_dir) == (768, 1024, 4, 9, "float16", "i.txt", "d")
    for bad in (["--registry", "reg.tsv"], ["--requests", "r.tsv"], ["--requests", "r", "--registry", "g", "--l", "3"], ["--requests", "r", "--registry", "g", "--dtype", "int8"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_requests_file_reader(tmp_path):
    f = tmp_path / "requests.tsv"
    f.write_text(f"alice\talice@example\n\nbob\tbob\t{KEY}\t{NONCE}\ncarol\tcarol\t{KEY}\t\ndave\tdave\t\t\n")
    reqs = issue.read_requests(f)
    assert [r.user_id for r in reqs] == ["alice", "bob", "carol", "dave"] and [r.message for r in reqs] == ["alice@example", "bob", "carol", "dave"]
    assert (reqs[1].key, reqs[1].nonce) == (bytes.fromhex(KEY), bytes.fromhex(NONCE))
    assert (reqs[2].key, reqs[2].nonce) == (bytes.fromhex(KEY), bytes.fromhex(KEY[16:48]))
    assert reqs[0].key != reqs[3].key and len(reqs[3].key) == 32
    f.write_text(f"alice\talice@example\nbob\tbob\t{KEY}\n")
    with pytest.raises(ValueError, match=r"requests\.tsv:2: .*got 3 columns"):
        issue.read_requests(f)
    f.write_text("alice\n")
    with pytest.raises(ValueError, match=r"requests\.tsv:1: .*got 1 columns"):
        issue.read_requests(f)
    f.write_text(f"alice\tm\t{KEY[:-2]}\t{NONCE}\n")
    with pytest.raises(ValueError, match=r"requests\.tsv:1: user 'alice'.*32 bytes"):
        issue.read_requests(f)
    f.write_text("\n\n")
    with pytest.raises(ValueError, match="no requests"):
        issue.read_requests(f)


def test_main_refuses_a_clash_before_loading_torch_or_writing(tmp_path, monkeypatch):
    reg = _registry()
    reg.save(tmp_path / "reg.tsv")
    before = open(tmp_path / "reg.tsv").read()
    (tmp_path / "r.tsv").write_text("alice\tnot her message\n")
    monkeypatch.setattr(issue, "issue_latents", lambda *a, **k: (_ for _ in ()).throw(AssertionError("reached the device")))
    with pytest.raises(ValueError, match="'alice' is already bound"):
        issue.main(["--requests", str(tmp_path / "r.tsv"), "--registry", str(tmp_path / "reg.tsv"), "--info_data", str(tmp_path / "i.txt"), "--out_dir", str(tmp_path / "o")])
    assert open(tmp_path / "reg.tsv").read() == before and not (tmp_path / "i.txt").exists() and not (tmp_path / "o").exists()
    with pytest.raises(ValueError, match="multiples of 8"):
        issue.main(["--requests", str(tmp_path / "r.tsv"), "--registry", str(tmp_path / "reg.tsv"), "--height", "500"])


def test_latent_file_names():
    assert issue.latent_file_names(["alice", "a/b", "a b", "alice", "..", "ünï"]) == ["alice.npy", "a_b.npy", "a_b.2.npy", "alice.2.npy", "_.npy", "_n_.npy"]


def test_issue_does_not_import_the_oracle():
    src = open(os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "issue.py")).read()
    names = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Import):
            names |= {a.name for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add(("." * node.level) + (node.module or ""))
            names |= {a.name for a in node.names}
    assert not any("oracle" in n for n in names), names
    assert "gs_oracle" not in src and "image_oracle" not in src
