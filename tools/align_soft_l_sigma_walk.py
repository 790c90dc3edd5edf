"""profiles/align_soft_l_sigma_walk.txt: the choice of the noise for the end-to-end tests of DESIGN.md section 4.28, on the CPU restatement alone
(tests/align_soft_l_reference.py; no device).  For l = 2 and 4, sigma = 0.25, 0.5, .. 10 and each of the three searches (detect over a 12-key ring, the shared-key
trace and the keyed trace over 1000 records; six 4 x 32 x 32 latents, 200 alignments, fpr 1e-6) one line: how many of the six the 15-level statistic names rightly
and wrongly, the range of its bounds, and the same for the sign search.

    python tools/align_soft_l_sigma_walk.py > profiles/align_soft_l_sigma_walk.txt          (about ten minutes on one core)"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import gswm_amd  # noqa: E402,F401
from gswm_amd import align as AL, detect as D, soft as S, trace as T  # noqa: E402

import align_soft_l_reference as ALR  # noqa: E402
import trace_align_reference as TR  # noqa: E402

E = ALR.E2E
limit = math.log10(E["fpr"])
cands = AL.alignments("d4", E["shift"], E["shape"][1], E["shape"][2])
want_al = ALR.restoring(cands)
n = E["shape"][0] * E["shape"][1] * E["shape"][2]
print("l\tsigma\tsearch\tlevels right\tlevels wrong\tlevels log10 p\tsigns right\tsigns wrong\tsigns log10 p")
gaps = []
for l in (2, 4):
    s = ALR.e2e_setup(l)
    cw = TR.codewords(s["records"], n * l)
    for i in range(1, 41):
        sigma = 0.25 * i
        for search in ("detect", "shared", "keyed"):
            r = ALR.e2e_host(search, s, l, sigma, cands, cw, (S, T, D))
            lev, sig = (ALR.named(r[k], r["rows"], want_al, limit) for k in ("levels", "signs"))
            span = lambda res: f"{min(h[3] for h in res):.1f} .. {max(h[3] for h in res):.1f}"
            print(f"{l}\t{sigma}\t{search}\t{lev[0]}\t{lev[1]}\t{span(r['levels'])}\t{sig[0]}\t{sig[1]}\t{span(r['signs'])}", flush=True)
            if lev == (6, 0) and sig[0] < 6 and sig[1] == 0:
                gaps.append((l, sigma, search))
print("# (l, sigma, search) at which the levels name all six and the signs fewer, neither a wrong one:", gaps if gaps else "none on this grid")
