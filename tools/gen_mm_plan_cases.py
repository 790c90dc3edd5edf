"""Input columns of tests/golden/mm_plan_cases.tsv: one matmul-engine launch per row, as mm_decide (csrc/gswm_mm_plan.h) sees it.

    python tools/gen_mm_plan_cases.py > inputs.tsv

The decision columns of the committed table are NOT written here: they record what the engine decided for these rows before the policy became one function
(and, after a deliberate change of policy, what the new policy decides -- the diff of the table is the change).  tests/mm_plan_cases.cpp prints them for the
current policy; tests/test_mm_plan_host.py compares and counts the coverage by the tags in the first column.

Pointers are given as 0 (null), 1 (aligned) or 2 (misaligned); `present` operands as 0 / 1.  Knobs outside the columns are the defaults (256 CUs, no A/B value set)."""
import sys

DENSE, PF, TOK2PF, UP2X, GEGLU, TRANS, QKV = range(7)
F16, BF16 = 1, 2
COLS = ("tag mode M N P nseg ld_max ldw ldy ldr resid rowbias ln_stat bias flags Hp Wp in_Hp in_Wp S n_rows y2 ws_ptr ws_bytes max_splits cs_ptr cs_cap rs_ptr rs_cap "
        "ex_flags tile_rows split_mask dtype").split()
WS = 40 << 20
rows = []


def row(tag, mode, M, N, P, **kw):
    r = dict(tag=tag, mode=mode, M=M, N=N, P=P, nseg=1, ld_max=64 * P, ldw=64 * P, ldy=N // 2 if mode == GEGLU else N, ldr=N // 2 if mode == GEGLU else N,
             resid=0, rowbias=0, ln_stat=0, bias=1, flags=0, Hp=1, Wp=1, in_Hp=1, in_Wp=1, S=1, n_rows=0, y2=0, ws_ptr=1, ws_bytes=WS, max_splits=0,
             cs_ptr=0, cs_cap=0, rs_ptr=0, rs_cap=0, ex_flags=0, tile_rows=0, split_mask=10, dtype=F16)
    assert not set(kw) - set(r), set(kw) - set(r)
    r.update(kw)
    rows.append(r)
    return r


def conv(tag, B, H, C, N, taps=9, compact=1, stride=1, up=0, C1=0, C2=0, **kw):
    """a convolution launch as gswm_conv.hip's launch_engine prepares it: output H x H per image, padded-flat rows"""
    Hp = H + 2
    inHp = H * stride + 2
    M = B * H * H if compact else B * Hp * Hp
    P = taps * (C // 64) + C1 // 64 + C2 // 64
    cs = {}
    if compact:          # the record buffer pf.py arms: 32-row blocks of 128-row tiles
        cs = dict(cs_ptr=1, cs_cap=(M + 127) // 128 * 4 * N)
    cs.update(kw)
    return row(tag, UP2X if up else PF, M, N, P, nseg=1 + (C1 > 0) + (C2 > 0), ld_max=max(C, C1, C2), ldw=taps * C + C1 + C2, flags=compact,
               Hp=Hp, Wp=Hp, in_Hp=inHp, in_Wp=inHp, **cs)


def rs(M, N):
    return dict(rs_ptr=1, rs_cap=M * 2 * ((N + 159) // 160) * 2)


# ---- the launches of an SD 2.1 forward (UNet levels 64x64x320, 32x32x640, 16x16x1280, 8x8x1280; context 77 -> 80 rows x 1024) ----------------------------------
LEVELS = ((64, 320), (32, 640), (16, 1280), (8, 1280))
for B in (1, 2, 8, 16, 64, 128):
    for H, C in LEVELS:
        M, S, t = B * H * H, H * H, f"sd21/b{B}/{H}x{H}x{C}"
        row(t + "/proj_in", DENSE, M, C, C // 64, **rs(M, C))
        row(t + "/qkv", QKV, M, 3 * C, C // 64, n_rows=2 * C, y2=1, ldy=2 * C, ldr=2 * C, S=S, bias=0)
        row(t + "/v_trans", TRANS, M, C, C // 64, S=S, bias=0)
        row(t + "/geglu_ln", GEGLU, M, 8 * C, C // 64, ln_stat=1, bias=0)
        row(t + "/ffout_proj_out_2seg", TOK2PF, M, C, 5 * C // 64, nseg=2, ld_max=4 * C, resid=1, S=S, Hp=H + 2, Wp=H + 2, cs_ptr=1, cs_cap=(M + 127) // 128 * 4 * C)
        row(t + "/proj_out_scatter", TOK2PF, M, C, C // 64, resid=1, S=S, Hp=H + 2, Wp=H + 2, cs_ptr=1, cs_cap=(M + 127) // 128 * 4 * C)
        for compact in (0, 1):
            e = "/int" if compact else "/pad"
            conv(t + "/conv3x3" + e, B, H, C, C, compact=compact, rowbias=1)
            conv(t + "/conv1x1" + e, B, H, C, C, taps=1, compact=compact)
            conv(t + "/shortcut_2seg" + e, B, H, C, C, C1=C // 2 if C > 320 else C, compact=compact)
            conv(t + "/shortcut_3seg" + e, B, H, C, C, C1=C, C2=C // 2 if H > 8 else C, compact=compact)
            if H > 8:
                conv(t + "/down_stride2" + e, B, H // 2, C, C, stride=2, compact=compact)
            if H < 64:
                conv(t + "/up2x" + e, B, H, C, C, taps=4, up=1, compact=compact)
# the VAE decoder's convolutions (output 128 / 256 / 512 channels) at 1 and 8 images
for B in (1, 8):
    for H, C, N in ((64, 512, 512), (128, 512, 512), (256, 512, 256), (256, 256, 256), (512, 256, 128), (512, 128, 128)):
        conv(f"vae/b{B}/{H}x{H}/{C}to{N}", B, H, C, N)
    for H, C in ((64, 512), (128, 512), (256, 256)):
        conv(f"vae/b{B}/{H}x{H}/up2x_{C}", B, H, C, C, taps=4, up=1)

# ---- the policy's branches -------------------------------------------------------------------------------------------------------------------------------
big = dict(M=65536, N=1280, P=20)
row("cover/wide/taken_dense", DENSE, **big)
row("cover/wide/taken_geglu", GEGLU, 32768, 2560, 5)
conv("cover/wide/taken_pf", 16, 64, 640, 1280)
row("cover/wide/refused_mode_trans", TRANS, S=4096, **big)
row("cover/wide/refused_mode_qkv", QKV, 65536, 1920, 20, n_rows=1280, y2=1, S=4096)
row("cover/wide/refused_n320", DENSE, 65536, 1440, 20)
row("cover/wide/refused_m256_dense", DENSE, 65536 + 128, 1280, 20)
row("cover/wide/refused_m256_geglu", GEGLU, 32768 + 128, 2560, 5)
row("cover/wide/m256_does_not_bind_pf", TOK2PF, 65536 + 128, 1280, 64, S=4096, Hp=66, Wp=66)
for name, key, lo, hi in (("resid", "ldr", 32752, 32760), ("y", "ldy", 32752, 32760), ("a", "ld_max", 32752, 32760), ("w", "ldw", 1677304, 1677312)):
    for side, v in (("below", lo), ("at", hi)):
        row(f"cover/wide/bound_{name}_{side}", DENSE, resid=1 if name == "resid" else 0, **{key: v}, **big)
row("cover/wide/pmin_dense_below", DENSE, 65536, 1280, 4)
row("cover/wide/pmin_dense_at", DENSE, 65536, 1280, 5)
row("cover/wide/pmin_res_below", DENSE, 65536, 1280, 7, resid=1)
row("cover/wide/pmin_res_at", DENSE, 65536, 1280, 8, resid=1)
conv("cover/wide/pmin_pf_below", 16, 64, 448, 1280)
conv("cover/wide/pmin_pf_at", 16, 64, 448, 1280, C1=64)
row("cover/wide/refused_fewer_tiles_than_cus", DENSE, 12800, 1600, 20)
row("cover/wide/refused_rounds", DENSE, 36864, 1280, 20)
row("cover/wide/refused_m_below_2048", DENSE, 1024, 40960, 5)
row("cover/wide/m_at_2048", DENSE, 2048, 40960, 5)
row("cover/wide/refused_two_segments", DENSE, nseg=2, **big)
row("cover/wide/two_segments_forced_512", DENSE, nseg=2, tile_rows=512, **big)
row("cover/wide/two_segments_pf_taken", TOK2PF, 65536, 1280, 64, nseg=2, S=4096, Hp=66, Wp=66)
row("cover/wide/forced_512", DENSE, 4096, 640, 5, tile_rows=512)
row("cover/wide/forced_512_illegal", DENSE, 4096, 800, 5, tile_rows=512)
row("cover/wide/forced_256", DENSE, tile_rows=256, **big)
row("cover/wide/forced_128", DENSE, tile_rows=128, **big)
# split-K: the automatic plan over the deep levels' shapes, forced splits, workspace too small / absent, max_splits 1
for M in (64, 256, 1156, 4096):
    for N in (320, 1280):
        for P in (8, 20, 64, 90, 360):
            conv_like = dict(Hp=10, Wp=10, in_Hp=10, in_Wp=10)
            row(f"cover/split/auto/{M}x{N}x{P}", PF, M, N, P, **conv_like)
for tr in (0, 128, 256):
    for ms in (2, 4, 7, 64):
        row(f"cover/split/forced_{ms}/bm{tr}", DENSE, 320, 640, 20, max_splits=ms, tile_rows=tr)
    row(f"cover/split/auto/bm{tr}", PF, 1024, 1280, 180, tile_rows=tr, Hp=10, Wp=10, in_Hp=10, in_Wp=10)
row("cover/split/forced_few_stages", DENSE, 320, 640, 1, max_splits=8)
row("cover/split/forced_chip_full", DENSE, 32768, 1280, 20, max_splits=8)
row("cover/split/workspace_too_small", PF, 64, 1280, 180, ws_bytes=1 << 20, Hp=10, Wp=10, in_Hp=10, in_Wp=10)
row("cover/split/workspace_one_byte_short", PF, 64, 1280, 180, ws_bytes=30 * 8 * 8 * 5 * 2 * 64 * 16 - 1, Hp=10, Wp=10, in_Hp=10, in_Wp=10)
row("cover/split/workspace_exact", PF, 64, 1280, 180, ws_bytes=30 * 8 * 8 * 5 * 2 * 64 * 16, Hp=10, Wp=10, in_Hp=10, in_Wp=10)
row("cover/split/no_workspace_null", PF, 64, 1280, 180, ws_ptr=0, Hp=10, Wp=10, in_Hp=10, in_Wp=10)
row("cover/split/no_workspace_zero_bytes", PF, 64, 1280, 180, ws_bytes=0, Hp=10, Wp=10, in_Hp=10, in_Wp=10)
row("cover/split/max_splits_1", PF, 64, 1280, 180, max_splits=1, Hp=10, Wp=10, in_Hp=10, in_Wp=10)
row("cover/split/ln_stat_never_splits", DENSE, 64, 1280, 180, ln_stat=1, bias=0)
# panels
row("cover/panel/8", DENSE, 4096, 1280, 20)
row("cover/panel/all_narrow_tiles", DENSE, 4096, 1600, 5)
row("cover/panel/narrow_over_budget", DENSE, 4096, 1600, 11)
row("cover/panel/4", DENSE, **big)
row("cover/panel/all_wide_tiles", GEGLU, 32768, 2560, 5)
# epilogue kinds x the 12-wave form through the split mask x tile rows
for mask in (0, 15):
    for tr in (128, 256):
        k = dict(split_mask=mask, tile_rows=tr, max_splits=1)
        row(f"cover/form/epi0/mask{mask}/bm{tr}", DENSE, 4096, 640, 10, **k)
        row(f"cover/form/epi1/mask{mask}/bm{tr}", PF, 4096, 640, 10, Hp=66, Wp=66, in_Hp=66, in_Wp=66, flags=1, **k)
        row(f"cover/form/epi1_rowbias_dense/mask{mask}/bm{tr}", DENSE, 4096, 640, 10, rowbias=1, **k)
        row(f"cover/form/epi2/mask{mask}/bm{tr}", GEGLU, 4096, 640, 10, **k)
        row(f"cover/form/epi3/mask{mask}/bm{tr}", TRANS, 4096, 640, 10, S=4096, **k)
        row(f"cover/form/epi5/mask{mask}/bm{tr}", QKV, 4096, 960, 10, n_rows=640, y2=1, S=4096, **k)
        row(f"cover/form/lnf/mask{mask}/bm{tr}", DENSE, 4096, 640, 10, ln_stat=1, bias=0, **k)
    row(f"cover/form/wide/mask{mask}", DENSE, split_mask=mask, **big)
    row(f"cover/form/splitk/mask{mask}", PF, 64, 1280, 180, split_mask=mask, Hp=10, Wp=10, in_Hp=10, in_Wp=10)
row("cover/form/bf16", DENSE, 4096, 640, 10, dtype=BF16)
# LayerNorm folded at MT 2, 4, 8
row("cover/lnf/mt2", DENSE, 1024, 640, 10, ln_stat=1, bias=0)
row("cover/lnf/mt4", DENSE, 65536, 1440, 20, ln_stat=1, bias=0)
row("cover/lnf/mt8", DENSE, ln_stat=1, bias=0, **big)
row("cover/lnf/mt8_geglu", GEGLU, 32768, 2560, 5, ln_stat=1, bias=0)
row("cover/lnf/trans_mt2", TRANS, 1024, 640, 10, ln_stat=1, bias=0, S=1024)
# records: granted at the exact capacity, refused one float short
for name, M, N, P in (("narrow", 4096, 640, 10), ("wide", 65536, 1280, 20)):
    slots = N // 80 if name == "wide" else 2 * ((N + 159) // 160)
    row(f"cover/rowstats/{name}_granted", DENSE, M, N, P, rs_ptr=1, rs_cap=M * slots * 2)
    row(f"cover/rowstats/{name}_one_short", DENSE, M, N, P, rs_ptr=1, rs_cap=M * slots * 2 - 1)
row("cover/rowstats/null_pointer", DENSE, 4096, 640, 10, rs_ptr=0, rs_cap=1 << 30)
row("cover/rowstats/not_for_rowbias", DENSE, 4096, 640, 10, rowbias=1, rs_ptr=1, rs_cap=1 << 30)
row("cover/rowstats/not_for_ln", DENSE, 4096, 640, 10, ln_stat=1, bias=0, rs_ptr=1, rs_cap=1 << 30)
row("cover/rowstats/not_for_geglu", GEGLU, 4096, 640, 10, rs_ptr=1, rs_cap=1 << 30)
for name, M, N, P, bm, wmv in (("narrow128", 4096, 640, 10, 128, 4), ("narrow256", 65536, 640, 10, 256, 4), ("wide", 65536, 1280, 64, 256, 2)):
    cap = (M + bm - 1) // bm * wmv * N
    g = dict(S=4096, Hp=66, Wp=66)
    row(f"cover/colstats/{name}_granted", TOK2PF, M, N, P, cs_ptr=1, cs_cap=cap, **g)
    row(f"cover/colstats/{name}_one_short", TOK2PF, M, N, P, cs_ptr=1, cs_cap=cap - 1, **g)
row("cover/colstats/null_pointer", TOK2PF, 4096, 640, 10, cs_ptr=0, cs_cap=1 << 30, S=4096, Hp=66, Wp=66)
conv("cover/colstats/not_for_padded_rows", 1, 64, 640, 640, compact=0, cs_ptr=1, cs_cap=1 << 30)
conv("cover/colstats/up2x_interior", 8, 32, 640, 640, taps=4, up=1, cs_ptr=1, cs_cap=1 << 30)
row("cover/colstats/not_for_dense", DENSE, 4096, 640, 10, cs_ptr=1, cs_cap=1 << 30)
row("cover/colstats/not_when_split", PF, 64, 1280, 180, flags=1, cs_ptr=1, cs_cap=1 << 30, Hp=10, Wp=10, in_Hp=10, in_Wp=10)
# every early error return, in the order of the checks, and pairs that fix which code wins
ok = dict(mode=DENSE, M=4096, N=640, P=10)
row("err/dtype", dtype=0, **ok)
row("err/dtype_f64", dtype=3, **ok)
row("err/colstats_capacity_negative", cs_cap=-1, **ok)
row("err/rowstats_capacity_negative", rs_cap=-1, **ok)
row("err/workspace_bytes_negative", ws_bytes=-1, **ok)
row("err/max_splits_negative", max_splits=-1, **ok)
row("err/max_splits_above_64", max_splits=65, **ok)
row("err/colstats_misaligned", cs_ptr=2, cs_cap=16, **ok)
row("err/rowstats_misaligned", rs_ptr=2, rs_cap=16, **ok)
row("err/workspace_misaligned", ws_ptr=2, **ok)
row("err/unknown_flag_bits", ex_flags=2, **ok)
row("err/n_mod_8", DENSE, 4096, 644, 10)
row("err/geglu_n_mod_160", GEGLU, 4096, 648, 10)
row("err/m_zero", DENSE, 0, 640, 10)
row("err/p_zero", DENSE, 4096, 640, 0)
row("err/qkv_n_rows_zero", QKV, 4096, 960, 10, n_rows=0, y2=1)
row("err/qkv_n_rows_mod_160", QKV, 4096, 960, 10, n_rows=648, y2=1)
row("err/qkv_n_rows_all", QKV, 4096, 960, 10, n_rows=960, y2=1)
row("err/qkv_no_y2", QKV, 4096, 960, 10, n_rows=640, y2=0)
row("err/bias_misaligned_dense", bias=2, **ok)
row("err/bias_misaligned_geglu", GEGLU, 4096, 640, 10, bias=2)
row("err/ln_stat_mode", PF, 4096, 640, 10, ln_stat=1, Hp=66, Wp=66, in_Hp=66, in_Wp=66)
row("err/ln_stat_rowbias", DENSE, 4096, 640, 10, ln_stat=1, rowbias=1)
row("err/wide_forced_two_segments", DENSE, nseg=2, tile_rows=512, **big)
row("err/too_many_tiles", DENSE, 0x7FFFFF00, 41120, 5)
row("err/order/dtype_before_n_mod_8", DENSE, 4096, 644, 10, dtype=0)
row("err/order/extras_before_n_mod_8", DENSE, 4096, 644, 10, max_splits=65)
row("err/order/n_mod_8_before_bias", DENSE, 4096, 644, 10, bias=2)
row("err/order/bias_before_ln_stat_rowbias", DENSE, 4096, 640, 10, bias=2, ln_stat=1, rowbias=1)
row("err/order/bias_ok_for_pf_rows", PF, 4096, 640, 10, bias=2, Hp=66, Wp=66, in_Hp=66, in_Wp=66)

tags = [r["tag"] for r in rows]
assert len(set(tags)) == len(tags), [t for t in tags if tags.count(t) > 1][:5]
sys.stdout.write("\t".join(COLS) + "\n")
for r in rows:
    sys.stdout.write("\t".join(str(r[c]) for c in COLS) + "\n")
