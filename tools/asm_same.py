#!/usr/bin/env python3
"""Is the device code of two builds the same?  Runs on the CPU.

  make -C embedded-qp-solver_amd asm        (in both trees)
  python tools/asm_same.py A/build/asm B/build/asm [qpb_gi.s ...]

Both listings are normalised -- comment lines, blank lines and the .file /
.loc / .ident lines dropped, the hash in the name of the __hip_cuid_ marker
(it follows the source text) blanked -- and everything that is left is compared: the
instructions, the .amdhsa_* block and the .set lines of every kernel, and the
rest of the file (its head and the metadata notes).  One line per kernel
symbol: same / DIFFERENT, VGPRs, scratch bytes, LDS bytes (`a -> b` where they
differ).  Exit status 1 on any difference."""
import os
import re
import sys

DROP = re.compile(r"^\s*(;|\.file\b|\.loc\b|\.ident\b|$)")
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")  # a one-byte object named by a hash of the source text
HEAD = re.compile(r"^\s*\.(section|protected|globl|weak|hidden|p2align|type)\b")
FIGURES = (("vgpr", "next_free_vgpr"), ("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size"))


def split(path):
    """-> {kernel symbol: its lines}, the lines outside every kernel."""
    lines = [CUID.sub("__hip_cuid_", l.rstrip()) for l in open(path) if not DROP.match(l)]
    starts = []
    for sym in re.findall(r"^\s*\.amdhsa_kernel (\S+)$", "\n".join(lines), re.M):
        at = next(i for i, l in enumerate(lines) if l.split(";")[0].strip() == sym + ":")
        while at > 0 and HEAD.match(lines[at - 1]):
            at -= 1
        starts.append((at, sym))
    starts.sort()
    end = next((i for i, l in enumerate(lines) if l.strip().startswith(".amdgpu_metadata")), len(lines))
    kernels = {}
    for (at, sym), (nxt, _) in zip(starts, starts[1:] + [(end, None)]):
        kernels[sym] = lines[at:nxt]
    rest = lines[:starts[0][0]] + lines[end:] if starts else lines
    return kernels, rest


def figures(seg):
    text = "\n".join(seg)
    return {k: (m.group(1) if (m := re.search(r"\.amdhsa_" + d + r" (\d+)", text)) else "?") for k, d in FIGURES}


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    a, b = sys.argv[1:3]
    names = sys.argv[3:] or sorted({f for d in (a, b) for f in os.listdir(d) if f.endswith(".s")})
    differ = 0
    for name in names:
        pa, pb = os.path.join(a, name), os.path.join(b, name)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"DIFFERENT  {name}: in one build only")
            differ += 1
            continue
        (ka, ra), (kb, rb) = split(pa), split(pb)
        print(f"{name}: {sum(map(len, ka.values())) + len(ra)} normalised lines")
        for sym in list(ka) + [s for s in kb if s not in ka]:
            sa, sb = ka.get(sym, []), kb.get(sym, [])
            fa, fb = figures(sa), figures(sb)
            same = sa == sb
            differ += not same
            fig = "  ".join(f"{k} {fa[k]}" if fa[k] == fb[k] else f"{k} {fa[k]} -> {fb[k]}" for k, _ in FIGURES)
            print(f"  {'same     ' if same else 'DIFFERENT'}  {fig}  {sym}")
        if ra != rb:
            print("  DIFFERENT  outside the kernels (file head, metadata)")
            differ += 1
    print("all the same" if not differ else f"{differ} different")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
