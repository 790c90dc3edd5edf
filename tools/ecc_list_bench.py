#!/usr/bin/env python3
"""The list read of error-corrected payloads (gsw_viterbi_list_decode, L = 1, 2, 4, 8) next to the plain read (gsw_viterbi_decode) on the same votes, both
forms of the list kernel's metric exchange, and the list walk through the device path.

    python tools/ecc_list_bench.py [--images 1 64 16384] [--rounds 20] [--reps 10] [--out profiles/ecc_list_bench.txt]

Speed.  Votes of B latents of 4x64x64 fp16 under their own records (gsw_extract_soft, 15 uniform levels), messages of M = 256 and M = 2048 bits.  One
process; per round every way runs once, one after the other (interleaved), on the same votes into buffers allocated before the first round: the C entry points
are called directly, `reps` launches back to back between two device events, the time of a way in a round is the events' time over `reps`.  The report is the
median over the rounds with the spread (min .. max), the ratio of each list size to the plain read of the same run, and whether L = 1 through the new entry
point lies within the plain read's spread.

Exchange.  The list kernel fetches the 2 L metrics of a state's two predecessors either through an LDS buffer of the wave (4 L bytes written, 8 L contiguous
bytes read per lane) or with 2 L ds_bpermute.  tools/viterbi_list_exchange.hip instantiates both for every L (built once into tools/build/libvlx.so with
hipcc); they are timed in the same rounds, and the report says which form the library ships.

Walk.  tools/ecc_list_sigma_walk.py's walk with the embed, the soft vote and the list read on the device: per sigma and L the payloads read back exactly with
ok, next to the CPU walk's count.  Needs a GPU."""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

LS = (1, 2, 4, 8)


def exchange_library(rebuild: bool):
    """tools/build/libvlx.so: both exchange forms of the list kernel at every L; built here when it is missing"""
    out = os.path.join(ROOT, "tools", "build", "libvlx.so")
    if rebuild or not os.path.isfile(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-fvisibility=hidden",
                               os.path.join(ROOT, "tools", "viterbi_list_exchange.hip"), "-o", out])
    lib = ctypes.CDLL(out)
    C = ctypes
    lib.vlx_decode.restype = C.c_int
    lib.vlx_decode.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8
    lib.vlx_shipped.restype = C.c_int
    lib.vlx_shipped.argtypes = [C.c_int]
    return lib


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, nargs="+", default=[1, 64, 16384])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rebuild", action="store_true", help="compile tools/viterbi_list_exchange.hip again")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ecc_list_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import gswm_amd  # noqa: F401
    from gswm_amd import _native as N, codec, ecc, soft
    import ecc_list_reference as LR
    import ecc_reference as R
    if not torch.cuda.is_available():
        raise SystemExit("ecc_list_bench: no GPU; nothing is measured on a CPU")
    vlx = exchange_library(a.rebuild)
    lib = N.lib()
    stream = codec._stream_ptr()
    shape = (4, 64, 64)
    shipped = {L: "lds" if vlx.vlx_shipped(L) else "bpermute" for L in LS}
    lines = [f"# tools/ecc_list_bench.py --images {' '.join(map(str, a.images))} --rounds {a.rounds} --reps {a.reps}: votes of B x 4x64x64 fp16 under their own "
             f"records, 15 uniform levels",
             f"# device: {torch.cuda.get_device_name(0)}; one process, the ways interleaved per round, {a.reps} launches between two device events, "
             f"median of {a.rounds} rounds (min .. max) of the time per launch",
             "# plain = gsw_viterbi_decode; L<n> = gsw_viterbi_list_decode as shipped (exchange: " + ", ".join(f"L = {L} {shipped[L]}" for L in LS) + "); "
             "L<n>/lds and L<n>/bperm = the same kernel with the metric exchange through LDS and with 2 L ds_bpermute (tools/viterbi_list_exchange.hip)",
             "#     M       B  way          median_us     min_us     max_us   us/image   vs_plain   results_equal"]
    all_ok = True
    summary = []
    for M in (256, 2048):
        mb, pb = M // 8, ecc.capacity(M)
        for B in a.images:
            rs = np.random.RandomState(B + M)
            payloads = [rs.bytes(pb) for _ in range(min(B, 64))]
            coded = [ecc.encode(p, M) for p in payloads]
            rows = np.zeros((B, codec.keyed_record_stride(mb)), dtype=np.uint8)
            rows[:, :48] = rs.randint(0, 256, (B, 48), dtype=np.uint8)
            rows[:, 48:48 + mb] = np.frombuffer(b"".join(coded[b % len(coded)] for b in range(B)), dtype=np.uint8).reshape(B, mb)
            records = torch.from_numpy(rows).cuda()
            z = codec.embed_records(records, mb, shape, seed=1, dtype=torch.float16, fast=True)
            z = (z.float() + 2.0 * torch.randn(z.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(B + M))).half() * (1.0 / 5.0 ** 0.5)
            score = codec.extract_soft(z, records, mb, soft.uniform_thresholds(z, 15)).score.contiguous()
            i32 = lambda: torch.empty((B,), dtype=torch.int32, device="cuda")
            outs = {}

            def buffers(w):
                outs[w] = (torch.empty((B, M // 16), dtype=torch.uint8, device="cuda"), torch.empty((B, M // 8), dtype=torch.uint8, device="cuda"),
                           i32(), i32(), i32(), i32(), i32())
                return [t.data_ptr() for t in outs[w]]

            calls = {}
            ptr = buffers("plain")
            calls["plain"] = lambda ptr=ptr: lib.gsw_viterbi_decode(score.data_ptr(), M, B, M, *ptr[:5], stream)
            for L in LS:
                ptr = buffers(f"L{L}")
                calls[f"L{L}"] = lambda ptr=ptr, L=L: lib.gsw_viterbi_list_decode(score.data_ptr(), M, B, M, L, *ptr, stream)
                for form, flag in (("lds", 1), ("bperm", 0)):
                    ptr = buffers(f"L{L}/{form}")
                    calls[f"L{L}/{form}"] = lambda ptr=ptr, L=L, flag=flag: vlx.vlx_decode(flag, score.data_ptr(), M, B, M, L, *ptr, stream)
            times = {w: [] for w in calls}
            for r in range(a.warmup + a.rounds):
                for w, call in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.reps):
                        st = call()
                    e1.record()
                    torch.cuda.synchronize()
                    if st != 0:
                        raise SystemExit(f"ecc_list_bench: {w} returned {st}")
                    if r >= a.warmup:
                        times[w].append(e0.elapsed_time(e1) * 1e-3 / a.reps)
            # what is timed is also right: L = 1 equals the plain read, both exchange forms equal the shipped kernel, a row of the batch equals the restatement
            equal = {"plain": True}
            for L in LS:
                ref = outs[f"L{L}"]
                equal[f"L{L}"] = all(torch.equal(x, y) for x, y in zip(ref[:5], outs["plain"][:5])) if L == 1 else True
                if B <= 64:
                    want = LR.decode_list(score.cpu().numpy()[:4], L)
                    equal[f"L{L}"] = equal[f"L{L}"] and all(np.array_equal(ref[i].cpu().numpy()[:4], want[n]) for i, n in enumerate(LR.NAMES))
                for form in ("lds", "bperm"):
                    equal[f"L{L}/{form}"] = all(torch.equal(x, y) for x, y in zip(ref, outs[f"L{L}/{form}"]))
            all_ok = all_ok and all(equal.values())
            med = {w: statistics.median(t) for w, t in times.items()}
            for w, t in times.items():
                lines.append(f"{M:>7} {B:>7}  {w:<10}  {med[w] * 1e6:>10.1f}  {min(t) * 1e6:>9.1f}  {max(t) * 1e6:>9.1f}  {med[w] * 1e6 / B:>9.3f}  "
                             f"{med[w] / med['plain']:>9.2f}   {equal[w]}")
            lo, hi = min(times["plain"]), max(times["plain"])
            summary.append(f"# M = {M}, B = {B}: list / plain = " + ", ".join(f"L = {L}: {med[f'L{L}'] / med['plain']:.2f}" for L in LS) +
                           f"; L = 1 through the new entry point is {'within' if lo <= med['L1'] <= hi else 'OUTSIDE'} the plain read's spread "
                           f"({med['L1'] * 1e6:.1f} us against {lo * 1e6:.1f} .. {hi * 1e6:.1f} us); exchange lds / bpermute: " +
                           ", ".join(f"L = {L}: {med[f'L{L}/lds'] * 1e6:.1f} / {med[f'L{L}/bperm'] * 1e6:.1f} us" for L in LS))
    lines += summary

    # ---- the walk through the device path
    W = R.WALK
    s = R.walk_setup()
    Bw, Mw = W["images"], W["M"]
    coded = [ecc.encode(p, Mw) for p in s["payloads"]]
    rows = np.zeros((Bw, codec.keyed_record_stride(Mw // 8)), dtype=np.uint8)
    rows[:, :48 + Mw // 8] = np.frombuffer(b"".join(s["keys"][b] + s["nonces"][b] + coded[b] for b in range(Bw)), dtype=np.uint8).reshape(Bw, -1)
    records = torch.from_numpy(rows).cuda()
    clean = codec.embed_records(records, Mw // 8, W["shape"], u=torch.from_numpy(s["u"]).cuda(), dtype=torch.float32)
    noise = torch.from_numpy(s["noise"]).cuda().view_as(clean)
    cpu = LR.walk_lists()
    lines += [f"# the walk of tools/ecc_list_sigma_walk.py through the device: embed_records, extract_soft with soft.uniform_thresholds (15 levels), "
              f"read_list; {Bw} images of {'x'.join(map(str, W['shape']))}, M = {Mw}; payloads read back exactly with ok, device / cpu",
              "#  sigma   " + "   ".join(f"L{L}_device/cpu" for L in LS)]
    walk_equal = True
    for i, sigma in enumerate(W["sigmas"]):
        zs = ((clean + sigma * noise) / (1.0 + sigma * sigma) ** 0.5).contiguous()
        score = codec.extract_soft(zs, records, Mw // 8, soft.uniform_thresholds(zs, W["levels"], W["clip"])).score
        cells = []
        for L in LS:
            read = ecc.read_list(score, L)
            got = sum(1 for b in range(Bw) if read.ok[b] and read.payload[b] == s["payloads"][b])
            walk_equal = walk_equal and got == cpu[L][0][i][1]
            cells.append(f"{got:>8} / {cpu[L][0][i][1]:<3}")
        lines.append(f"{sigma:>8.2f}   " + "   ".join(cells))
    lines.append(f"# the device walk {'equals' if walk_equal else 'DIFFERS from'} the CPU walk at every point and list size")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if all_ok and walk_equal else 1


if __name__ == "__main__":
    sys.exit(main())
