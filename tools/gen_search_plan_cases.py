"""Input columns of tests/golden/search_plan_cases.tsv: one search per row, as search_decide (csrc/gswm_search_plan.h) sees it.

    python tools/gen_search_plan_cases.py > inputs.tsv

The decision columns of the committed table are NOT written here: they record what the three entry points decided for these rows before the policy became one
function (and, after a deliberate change of policy, what the new policy decides -- the diff of the table is the change).  tests/search_plan_cases.cpp prints them
for the current policy; tests/test_search_plan_host.py compares and counts the coverage by the tags in the first column.

kind: 0 sign search, 1 level-weighted search, 2 key search.  Pointers are 0 (null), 1 (aligned) or 2 (misaligned: signs, planes and wsum off 4 bytes, records off
16); outs: 1 all there, 0 idx null, 2 score null, 3 workspace null."""
SIGN, LEVEL, KEY = range(3)
COLS = "tag kind B n_bits msg_bytes stride n_records k levels signs planes wsum records outs".split()
rows = []


def stride_of(kind, msg_bytes):
    return 48 if kind == KEY else (48 + msg_bytes + 15) // 16 * 16


def row(tag, kind, **kw):
    r = dict(tag=tag, kind=kind, B=4, n_bits=16384, msg_bytes=32, stride=None, n_records=1000, k=1, levels=15 if kind == LEVEL else 0, signs=1,
             planes=int(kind == LEVEL), wsum=int(kind == LEVEL), records=1, outs=1)
    assert not set(kw) - set(r), set(kw) - set(r)
    r.update(kw)
    if r["stride"] is None:
        r["stride"] = stride_of(kind, max(int(r["msg_bytes"]), 0))
    rows.append(r)


# ---- the record walks: every tile x message form, the tile shrinking by LDS --------------------------------------------------------------------------------------
for B, T in ((1, 1), (2, 4), (4, 4), (5, 16), (16, 16), (17, 64), (64, 64), (65, 64), (65535, 64)):
    for mb in (32, 3, 4, 5):
        row(f"cover/sign/b{B}_t{T}_mb{mb}", SIGN, B=B, msg_bytes=mb, n_bits=512 * 3 * 5 if mb in (3, 5) else 512)
for B in (64, 16, 4):
    for n_bits in (16384, 16640, 65536, 65792, 262144, 262400, 1048576):      # 64 -> 16 -> 4 -> 1 images, at each edge and one row length past it
        row(f"cover/sign/shrink_b{B}_n{n_bits}", SIGN, B=B, n_bits=n_bits)
for levels, P in ((1, 1), (2, 2), (3, 2), (4, 3), (7, 3), (8, 4), (15, 4)):
    for B in (1, 4, 16, 64):
        for mb in (32, 3):
            row(f"cover/level/l{levels}_p{P}_b{B}_mb{mb}", LEVEL, levels=levels, B=B, msg_bytes=mb, n_bits=768 if mb == 3 else 512)
    edge = 131072 * 8 // (1 + P) // 64 // 64 * 64                                # bits of the longest row of which 64 images x (1 + P) rows fit
    for B in (64, 16, 4):
        for n_bits in (edge, edge + 512, 4 * edge, 4 * edge + 512, 16 * edge, 16 * edge + 512):
            row(f"cover/level/shrink_l{levels}_b{B}_n{n_bits}", LEVEL, levels=levels, B=B, n_bits=n_bits, msg_bytes=1)
# the level search's domain n_bits (1 + P) <= 1 048 576: the last admissible lattice of one-byte messages and the next
for levels, P in ((1, 1), (3, 2), (7, 3), (15, 4)):
    at = 1048576 // (1 + P) // 8 * 8
    row(f"cover/level/domain_p{P}_at", LEVEL, levels=levels, B=1, n_bits=at, msg_bytes=1)
    row(f"cover/level/domain_p{P}_past", LEVEL, levels=levels, B=1, n_bits=at + 8, msg_bytes=1)
    row(f"cover/level/domain_p{P}_at_b64", LEVEL, levels=levels, B=64, n_bits=at, msg_bytes=1)

# ---- the key search ----------------------------------------------------------------------------------------------------------------------------------------------
for copies, PL in ((1, 4), (15, 4), (16, 8), (255, 8), (256, 12), (4095, 12), (4096, 16), (32768, 16)):
    for B in (1, 5):
        row(f"cover/key/copies{copies}_pl{PL}_b{B}", KEY, B=B, msg_bytes=4, n_bits=32 * copies)
row("cover/key/pl0_mb3", KEY, msg_bytes=3, n_bits=24 * 100)
row("cover/key/pl0_mb5_b1", KEY, B=1, msg_bytes=5, n_bits=40 * 100)
for mb in (4, 32, 3):
    step = 8 * mb * (8 if mb == 3 else 1)
    for n_bits in (523264 // step * step, 523264 // step * step + step, 1048576 // step * step):      # the last lattice whose row shares the LDS with a keystream, the next
        for signs in (1, 2):
            for B in (1, 3):
                row(f"cover/key/sg_mb{mb}_n{n_bits}_signs{signs}_b{B}", KEY, B=B, msg_bytes=mb, n_bits=n_bits, signs=signs)
for mb in (4, 8, 16, 32, 64, 128, 256, 1, 2, 3, 7):                              # G clipped by the units (message words, or positions) ...
    for B in (1, 4, 16, 64):                                                     # ... and by the tile
        row(f"cover/key/g_mb{mb}_b{B}", KEY, B=B, msg_bytes=mb, n_bits=8 * mb * 2 * 3 * 5 * 7)
for B in (4, 16, 64):                                                            # (short rows: the tile stays as large as the batch)
    row(f"cover/key/g_by_tile_mb256_b{B}", KEY, B=B, msg_bytes=256, n_bits=8 * 256 * 2)
for nblk in (1, 2, 3, 4, 7, 8):                                                 # the bank offset: odd and even block counts under every G
    for mb in (4, 8, 16, 32, 64, 128):
        row(f"cover/key/srow_nblk{nblk}_mb{mb}", KEY, B=1, msg_bytes=mb, n_bits=512 * nblk if 512 * nblk % (8 * mb) == 0 else 8 * mb * nblk)
for n_bits in (512, 4096, 16384, 65536, 262144, 523264):                         # kpi clipped by LDS
    for B in (1, 4, 64):
        row(f"cover/key/kpi_lds_n{n_bits}_b{B}", KEY, B=B, msg_bytes=4, n_bits=n_bits)
for U in (1, 2, 3, 255, 256, 257, 511, 512, 513, 5000, 131072, 131073, 2 ** 31 - 1):      # kpi clipped by the keys; grid_x below its cap and at it
    for B in (1, 64):
        row(f"cover/key/u{U}_b{B}", KEY, B=B, msg_bytes=4, n_bits=512, n_records=U)
for U in (1, 7, 8, 9, 4087, 4088, 4089, 4096, 4097, 100000, 2 ** 31 - 1):
    row(f"cover/sign/u{U}", SIGN, n_records=U)
    row(f"cover/level/u{U}", LEVEL, n_records=U)
for k in range(1, 9):
    for kind, name in ((SIGN, "sign"), (LEVEL, "level"), (KEY, "key")):
        row(f"cover/{name}/k{k}", kind, k=k, B=3, n_records=5)

# ---- every refusal, one row per cause, in each search ------------------------------------------------------------------------------------------------------------
for kind, name in ((SIGN, "sign"), (LEVEL, "level"), (KEY, "key")):
    e = f"err/{name}/"
    row(e + "signs_null", kind, signs=0)
    row(e + "idx_null", kind, outs=0)
    row(e + "score_null", kind, outs=2)
    row(e + "workspace_null", kind, outs=3)
    row(e + "b_zero", kind, B=0)
    row(e + "k_zero", kind, k=0)
    row(e + "k_nine", kind, k=9)
    row(e + "n_bits_zero", kind, n_bits=0)
    row(e + "records_2p31", kind, n_records=2 ** 31)
    row(e + "records_null", kind, records=0)
    row(e + "records_zero", kind, n_records=0)
    row(e + "msg_bytes_zero", kind, msg_bytes=0)
    row(e + "msg_bytes_257", kind, msg_bytes=257, n_bits=8 * 257, stride=320)
    row(e + "stride_short", kind, stride=32 if kind == KEY else 64)
    row(e + "stride_not_16", kind, stride=56 if kind == KEY else 88)
    row(e + "records_misaligned", kind, records=2)
    row(e + "ragged", kind, n_bits=16384 + 8)
    row(e + "n_bits_past_domain", kind, n_bits=1048576 + 256)
    row(e + "b_65536", kind, B=65536)
    row(e + "order/bad_arg_before_ragged", kind, n_bits=16384 + 8, k=9)
    row(e + "order/bad_stride_before_ragged", kind, n_bits=16384 + 8, stride=40)
    row(e + "order/ragged_before_unsupported", kind, n_bits=1048576 + 8, B=65536)
    row(e + "ok/signs_misaligned", kind, signs=2)                               # not a refusal: the rows are read byte by byte
    row(e + "ok/stride_with_room", kind, stride=4096)
row("err/key/ok/stride_48_holds_no_message", KEY, stride=48, msg_bytes=32)
row("err/level/planes_null", LEVEL, planes=0)
row("err/level/wsum_null", LEVEL, wsum=0)
row("err/level/levels_zero", LEVEL, levels=0)
row("err/level/levels_16", LEVEL, levels=16)
row("err/level/wsum_misaligned", LEVEL, wsum=2)
row("err/level/ok/planes_misaligned", LEVEL, planes=2)
row("err/level/n_bits_past_domain_of_p4", LEVEL, n_bits=262144)

# ---- a grid over the sizes in use: lattices of 4 x 64 x 64 .. 4 x 128 x 128 x l, messages of 3 .. 32 bytes, batches up to 100 ---------------------------------------
for B in (1, 2, 5, 17, 64, 100):
    for n_bits in (768, 3072, 16128, 65280, 261888, 523776, 1048320):             # multiples of 768: whole copies of 3-, 4- and 32-byte messages
        for mb in (3, 4, 32):
            row(f"grid/sign/b{B}_n{n_bits}_mb{mb}", SIGN, B=B, n_bits=n_bits, msg_bytes=mb)
            for U in (7, 5000):
                row(f"grid/key/b{B}_n{n_bits}_mb{mb}_u{U}", KEY, B=B, n_bits=n_bits, msg_bytes=mb, n_records=U)
            if n_bits <= 261888 and mb != 4:
                for levels in (1, 3, 7, 15):
                    row(f"grid/level/b{B}_n{n_bits}_mb{mb}_l{levels}", LEVEL, B=B, n_bits=n_bits, msg_bytes=mb, levels=levels)

assert len({r["tag"] for r in rows}) == len(rows)
print("\t".join(COLS))
for r in rows:
    print("\t".join(str(r[c]) for c in COLS))
