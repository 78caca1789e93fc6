#!/usr/bin/env python3
"""Compare the device assembly of two builds, kernel by kernel.

    make -C embedded-qp-solver_amd asm      (at each commit; copy build/asm aside)
    tools/asm_compare.py OLD_ASM_DIR NEW_ASM_DIR

For every kernel symbol of OLD (an `.amdhsa_kernel` name) the instruction text
between the symbol's label and its `s_endpgm`, and its `.amdhsa_*` resource
directives (registers, LDS, scratch), must be the same in NEW.  Labels and
comments are dropped, so the kernels may move inside a file.  A kernel template
that gained a trailing template parameter whose default is `false` (and a
kernel that became such a template) is the same kernel under a longer name:
it is found through its demangled name (c++filt, or $CXXFILT).  So is a kernel
template that gained a trailing template parameter pack, empty in the old
instantiations: another symbol with the same demangled name (a second such
pack behind a filled one only changes how c++filt spaces the closing `>`s).  Kernels that
only NEW has are counted.  Exit status 1 when a kernel of OLD changed or is gone.
"""
import os
import re
import subprocess
import sys

CXXFILT = os.environ.get("CXXFILT", "c++filt")


def demangled(names):
    """{symbol: demangled name without the return type} for a list of symbols."""
    if not names:
        return {}
    out = subprocess.run([CXXFILT] + list(names), capture_output=True, text=True, check=True).stdout.splitlines()
    # (c++filt closes a nested template argument list as `> >` or `>>` depending on
    # whether an empty pack follows it: one spelling)
    return {n: re.sub(r"^void ", "", d).replace("> >", ">>") for n, d in zip(names, out)}


def successor(name, old_dem, new_dem):
    """The symbol of NEW that is OLD's `name`: itself, or the one whose template
    argument list grew by a trailing `false`."""
    if name in new_dem:
        return name
    d = old_dem[name]
    head, paren, args = d.partition("(")
    grown = (head[:-1] + ", false>" if head.endswith(">") else head + "<false>") + paren + args
    for n, dn in new_dem.items():
        if dn == grown:
            return n
    # a template that gained a trailing parameter pack, empty here: another
    # symbol, the same demangled name
    for n, dn in new_dem.items():
        if dn == d:
            return n
    return None


def kernels(path):
    """{symbol: (instructions, resource directives)} of one .s file."""
    out = {}
    lines = open(path, errors="replace").read().splitlines()
    names = [m.group(1) for ln in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))]
    for name in names:
        body, res, state = [], [], 0
        for ln in lines:
            if state == 0 and ln.startswith(name + ":"):
                state = 1
                continue
            if state == 1:
                t = ln.split(";")[0].strip()
                if not t or t.endswith(":") or t.startswith("."):
                    continue
                # local labels are numbered per file: keep only the fact of a branch target
                body.append(re.sub(r"\.LBB\d+_\d+", ".LBB", t))
                if t == "s_endpgm":
                    state = 2
            if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(name) + r"\s*$", ln):
                state = 3
                continue
            if state == 3:
                if ".end_amdhsa_kernel" in ln:
                    state = 4
                else:
                    res.append(ln.strip())
        out[name] = (body, res)
    return out


def main():
    old_dir, new_dir = sys.argv[1:3]
    bad = 0
    for f in sorted(os.listdir(old_dir)):
        if not f.endswith(".s"):
            continue
        old = kernels(os.path.join(old_dir, f))
        newp = os.path.join(new_dir, f)
        new = kernels(newp) if os.path.exists(newp) else {}
        same, renamed = 0, 0
        old_dem, new_dem = demangled(list(old)), demangled(list(new))
        found = set()
        for name, (body, res) in old.items():
            succ = successor(name, old_dem, new_dem)
            if succ is None:
                print(f"{f}: {old_dem[name]}: GONE")
                bad += 1
                continue
            found.add(succ)
            renamed += succ != name
            if new[succ][0] != body:
                print(f"{f}: {old_dem[name]}: INSTRUCTIONS DIFFER ({len(body)} -> {len(new[succ][0])})")
                bad += 1
            elif new[succ][1] != res:
                print(f"{f}: {old_dem[name]}: RESOURCE USAGE DIFFERS")
                bad += 1
            else:
                same += 1
        print(f"{f}: {same} of {len(old)} kernels identical ({renamed} under a grown name), "
              f"{len(set(new) - found)} new")
    for f in sorted(set(os.listdir(new_dir)) - set(os.listdir(old_dir))):
        if f.endswith(".s"):
            print(f"{f}: new file, {len(kernels(os.path.join(new_dir, f)))} kernels")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
