"""Are the kernels of two device assembly files the same code?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden --cuda-device-only -S csrc/gswm_keyed.hip -o new.s     (and the same of the parent: old.s)
    python tools/isa_compare.py old.s new.s > profiles/search_refactor_isa.txt

Per kernel of either file: the instruction stream with comments and directives stripped and local labels renumbered in order of appearance, compared as text.
Columns: kernel, instructions, VGPRs (of the second file; both where they differ), same / different.  Exit status 1 if any kernel differs or is missing."""
import re
import sys


def kernels(path):
    """{kernel: (instruction lines, vgprs)} of an assembly file as the compiler writes it"""
    out, name, body = {}, None, []
    for raw in open(path):
        line = raw.split(";")[0].rstrip()
        m = re.match(r"^(\w+):\s*$", line)
        if name is None:
            if m and not m.group(1).startswith(".L"):
                name, body = m.group(1), []
            continue
        v = re.search(r";\s*NumVgprs:\s*(\d+)", raw)
        if v:
            labels = {}
            text = [re.sub(r"\.L\w+", lambda t: labels.setdefault(t.group(0), f".L{len(labels)}"), l) for l in body]
            out[name], name = (text, int(v.group(1))), None
            continue
        s = line.strip()
        if s and (not s.startswith(".") or s.startswith(".L") and s.endswith(":")):
            body.append(s)
    return out


def main(old_path, new_path):
    old, new = kernels(old_path), kernels(new_path)
    bad = 0
    print(f"# {len(old)} kernels in the first file, {len(new)} in the second")
    print("kernel\tinstructions\tvgprs\tverdict")
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            print(f"{k}\t-\t-\tonly in the {'second' if k in new else 'first'} file")
            bad += 1
            continue
        (to, vo), (tn, vn) = old[k], new[k]
        count = lambda t: sum(1 for l in t if not l.endswith(":"))
        same = to == tn and vo == vn
        bad += not same
        print(f"{k}\t{count(tn) if same else f'{count(to)} -> {count(tn)}'}\t{vn if vo == vn else f'{vo} -> {vn}'}\t{'same' if same else 'DIFFERENT'}")
    print(f"# {len(set(old) | set(new)) - bad} same, {bad} different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
