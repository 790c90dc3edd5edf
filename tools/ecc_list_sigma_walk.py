"""Where a list under the Viterbi read brings payloads back that the single best path loses: tools/ecc_sigma_walk.py's walk over the noise on the latent,
read at list sizes 1, 2, 4 and 8, on the CPU from the restatements alone (tests/ecc_list_reference.py, tests/ecc_reference.py, tests/soft_reference.py, the
oracle's embed) -- no GPU, no library.

    python tools/ecc_list_sigma_walk.py            # writes profiles/ecc_list_sigma_walk.txt

Setup (ecc_reference.WALK, unchanged): 4 x 32 x 32 latents, M = 256, l = 1, 15 uniform levels on each image's own RMS, sigma 0.5 .. 4.0 in steps of 0.25, 20
images per point under their own keys, one fixed seed; the same coded latents, uniforms, unit noise and votes at every list size.  Per point and list size:
the images whose 13-byte payload comes back exactly with `ok` (right), and the images with `ok` on any other payload (wrong); then the 64 unwatermarked
latents of the seed with `ok`.  The end-to-end tests use the LARGEST sigma at which all 20 payloads read back at L = 8 and fewer than 20 at L = 1."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ecc_list_reference as LR  # noqa: E402
import ecc_reference as R  # noqa: E402


def report(walks) -> str:
    W = R.WALK
    Ls = sorted(walks)
    lines = [f"# ecc list sigma walk: {'x'.join(str(s) for s in W['shape'])} latents, M = {W['M']}, l = 1, {W['levels']} uniform levels (clip {W['clip']}), "
             f"{W['images']} images per point, seed {W['seed']}",
             f"# right: {R.capacity(W['M'])}-byte payloads read back exactly with ok; wrong: images with ok on another payload; per list size L",
             "sigma\t" + "\t".join(f"right_L{L}" for L in Ls) + "\t" + "\t".join(f"wrong_L{L}" for L in Ls)]
    for i, s in enumerate(W["sigmas"]):
        lines.append(f"{s:.2f}\t" + "\t".join(str(walks[L][0][i][1]) for L in Ls) + "\t" + "\t".join(str(walks[L][0][i][2]) for L in Ls))
    lines.append("# blank latents with ok, of 64: " + ", ".join(f"L = {L}: {walks[L][1]}" for L in Ls))
    wrong = sum(w for L in Ls for _, _, w in walks[L][0])
    lines.append(f"# images with ok on a wrong payload, all points and list sizes: {wrong} ({'the condition on the input holds' if not wrong else 'the condition on the input FAILS'})")
    chosen = LR.chosen_sigma(walks)
    if chosen is None:
        lines.append(f"# no grid point reads all {W['images']} payloads back at L = 8 and fewer at L = 1: the list buys nothing this walk can show")
    else:
        at = {L: next(r for s, r, _ in walks[L][0] if s == chosen) for L in Ls}
        lines.append(f"# chosen sigma {chosen:.2f}: the largest point with all {W['images']} payloads at L = 8 and fewer at L = 1; read back there: "
                     + ", ".join(f"L = {L}: {at[L]}" for L in Ls))
    return "\n".join(lines) + "\n"


def main():
    text = report(LR.walk_lists())
    out = os.path.join(ROOT, "profiles", "ecc_list_sigma_walk.txt")
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
