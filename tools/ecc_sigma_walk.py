"""Where the convolutional code reads payloads back and the uncoded message no longer does: a walk over the noise on the latent, on the CPU from the
restatements alone (tests/ecc_reference.py, tests/soft_reference.py, the oracle's embed) -- no GPU, no library.

    python tools/ecc_sigma_walk.py            # writes profiles/ecc_sigma_walk.txt

Setup (ecc_reference.WALK): 4 x 32 x 32 latents, M = 256, l = 1, 15 uniform levels on each image's own RMS, sigma 0.5 .. 4.0 in steps of 0.25, 20 images per
point under their own keys, one fixed seed; the same uniforms and the same unit noise at every point.  Per point: the images whose 13-byte payload comes back
exactly with `ok`, and for the UNCODED alternative -- the same 13 bytes + CRC as a 128-bit message with twice the copies, read by the same soft vote -- the
images whose every bit is right.  The end-to-end tests use the LARGEST sigma at which all 20 coded payloads read back."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ecc_reference as R  # noqa: E402


def report(table) -> str:
    W = R.WALK
    lines = [f"# ecc sigma walk: {'x'.join(str(s) for s in W['shape'])} latents, M = {W['M']}, l = 1, {W['levels']} uniform levels (clip {W['clip']}), "
             f"{W['images']} images per point, seed {W['seed']}",
             f"# coded: {R.capacity(W['M'])}-byte payloads read back exactly with ok; uncoded: the same bytes + CRC as a {W['M'] // 2}-bit message, every bit right",
             "sigma\tcoded\tuncoded"]
    lines += [f"{s:.2f}\t{c}\t{u}" for s, c, u in table]
    chosen = R.chosen_sigma(table)
    if chosen is None:
        lines.append("# no grid point reads all coded payloads back")
    else:
        u = next(u for s, _, u in table if s == chosen)
        lines.append(f"# chosen sigma {chosen:.2f}: the largest point with all {W['images']} coded payloads; the uncoded alternative reads {u} of {W['images']} there "
                     f"({'at most half: the condition on the input holds' if 2 * u <= W['images'] else 'MORE than half: the condition on the input fails'})")
    return "\n".join(lines) + "\n"


def main():
    text = report(R.walk())
    out = os.path.join(ROOT, "profiles", "ecc_sigma_walk.txt")
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
