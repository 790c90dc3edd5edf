"""What the punctured payload codes cost in noise: tools/ecc_sigma_walk.py's walk over the noise on the latent, read under "conv" (rate 1/2), "conv23"
(2/3) and "conv34" (3/4) at list sizes 1, 2, 4 and 8, on the CPU from the restatements alone (tests/ecc_rate_reference.py, tests/ecc_list_reference.py,
tests/ecc_reference.py, tests/soft_reference.py, the oracle's embed) -- no GPU, no library.

    python tools/ecc_rate_sigma_walk.py            # writes profiles/ecc_rate_sigma_walk.txt

Setup (ecc_reference.WALK and walk_setup(), unchanged): 4 x 32 x 32 latents, M = 256, l = 1, 15 uniform levels on each image's own RMS, sigma 0.5 .. 4.0 in
steps of 0.25, 20 images per point under their own keys, the same uniforms and unit noise for every code.  The codes carry 13, 18 and 21 bytes, so each has a
recorded payload draw of its own (ecc_rate_reference.PAYLOAD_SEED).  Per point, code and list size: the images whose payload comes back exactly with `ok`
(right) and the images with `ok` on any other payload (wrong); then the 64 unwatermarked latents of the seed with `ok`; `ecc_reference.walk()`'s uncoded
column (13 bytes + CRC as a 128-bit message with twice the copies) next to them, for the reader.  The end-to-end tests use, per code, the LARGEST sigma at
which all 20 payloads read back at L = 1."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ecc_list_reference as LR  # noqa: E402
import ecc_rate_reference as Q  # noqa: E402
import ecc_reference as R  # noqa: E402


def walks_of_all_codes():
    """-> ({code: ecc_rate_reference.walk(code)}, [uncoded images read, per grid point])"""
    setup = R.walk_setup()
    return {code: Q.walk(code, setup) for code in Q.CODES}, [u for _, _, u in R.walk()]


def report(walks, uncoded) -> str:
    W = R.WALK
    Ls = LR.LIST_SIZES
    lines = [f"# ecc rate sigma walk: {'x'.join(str(s) for s in W['shape'])} latents, M = {W['M']}, l = 1, {W['levels']} uniform levels (clip {W['clip']}), "
             f"{W['images']} images per point, seed {W['seed']}; payload draws " + ", ".join(f"{c}: {Q.PAYLOAD_SEED[c]}" for c in Q.CODES),
             "# payload bytes: " + ", ".join(f"{c}: {Q.capacity(W['M'], c)}" for c in Q.CODES) + "; right: payloads read back exactly with ok, per list size L; "
             "wrong: images with ok on another payload, summed over the list sizes; uncoded: the 13-byte message without a code, every bit right",
             "sigma\t" + "\t".join(f"{c}_L{L}" for c in Q.CODES for L in Ls) + "\t" + "\t".join(f"{c}_wrong" for c in Q.CODES) + "\tuncoded"]
    for i, s in enumerate(W["sigmas"]):
        lines.append(f"{s:.2f}\t" + "\t".join(str(walks[c][L][0][i][1]) for c in Q.CODES for L in Ls) + "\t" +
                     "\t".join(str(sum(walks[c][L][0][i][2] for L in Ls)) for c in Q.CODES) + f"\t{uncoded[i]}")
    for c in Q.CODES:
        lines.append(f"# {c}: blank latents with ok, of 64: " + ", ".join(f"L = {L}: {walks[c][L][1]}" for L in Ls))
    wrong = sum(w for c in Q.CODES for L in Ls for _, _, w in walks[c][L][0])
    lines.append(f"# images with ok on a wrong payload, all points, codes and list sizes: {wrong} "
                 f"({'the condition on the input holds' if not wrong else 'the condition on the input FAILS'})")
    for c in Q.CODES:
        plain, lst = Q.chosen_sigmas(walks[c])
        text = f"# {c}: chosen sigma {plain:.2f}, the largest point with all {W['images']} payloads at L = 1" if plain is not None else f"# {c}: no point reads all"
        if lst is None:
            text += f"; no grid point reads all {W['images']} at L = 8 and fewer at L = 1: the list end-to-end tests run at the L = 1 point"
        else:
            at = {L: next(r for s, r, _ in walks[c][L][0] if s == lst) for L in Ls}
            text += f"; list point {lst:.2f} (all at L = 8, fewer at L = 1): " + ", ".join(f"L = {L}: {at[L]}" for L in Ls)
        lines.append(text)
    return "\n".join(lines) + "\n"


def main():
    text = report(*walks_of_all_codes())
    out = os.path.join(ROOT, "profiles", "ecc_rate_sigma_walk.txt")
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
