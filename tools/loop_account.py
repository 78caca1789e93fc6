#!/usr/bin/env python3
"""Where the n <= 16 active-set kernel's instructions execute: basic block x
opcode class x executions per wave, for one instantiation of gi_dense_kernel.
Runs on the CPU.  Beside the issue classes, every section has a row ADDR64 (64-bit
address arithmetic on the VALU) and READLANE (v_readlane / v_readfirstlane).

  static counts   a hipcc -S listing of csrc/qpb_gi.hip (the Makefile's flags
                  plus -gline-tables-only, which leaves the code as it is): the
                  inlined-at chain of every instruction names the line of
                  gi_group it came from, and anchor lines of the source (the
                  clk.tick() section marks and a few statements) split gi_group
                  into sections.  A block of a column-unrolled section whose DPP
                  broadcasts all read lane J is column J's block.
  execution       a lockstep replay of tools/gi_select_sim.py's traces (dual
  counts          steepest-edge rule, the kernel's formulation), four QPs per
                  wave as the kernel runs them.  Per trip: which rows select,
                  work, ADD or DROP; qmax (the back substitution's bound, stale
                  q of finished rows included, as the readlanes see it), qmin
                  over the working rows (the dead-column bound), whether q is
                  uniform, the q values present, the Givens steps of a DROP.

  python tools/loop_account.py [--source csrc/qpb_gi.hip] [--listing file.s]
         [--kernel REGEX] [--family box] [--count 2000] [--out file.json]

Calibration: the total VALU per wave of the table is compared with the PMC's
SQ_INSTS_VALU per wave when --pmc-valu is given (2 993 for gi_dense v11.5 on
the box family); more than 5 % apart means the section-to-trip mapping below
is wrong for that listing."""
import argparse
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

FLAGSHIP = r"_ZN3qpb15gi_dense_kernelILi2ELb1ELb1ELb0ELi3E"
# issue cycles per wave64 instruction and class (bench.py's VALU_COST, tools/probe/valu_probe.hip)
VALU_COST = {"FMA_F64": 5.24, "MUL_F64": 5.47, "ADD_F64": 5.47, "TRANS_F64": 17.23, "B32": 3.07}
NL = 16

# (section, the first source line at or after the previous anchor that contains this text)
ANCHORS = [
    ("setup", "SectionClock<STAMP> clk"),
    ("loop_head", "while (!done && it < max_iter) {"),
    ("select", "if (selecting) {"),
    ("exchange", "clk.tick(4);"),
    ("slack_product", "bdot_rows<MR>(d2, E, u"),
    ("norm_d2", "const double nd2 = row_sum"),
    ("back_subst", "clk.tick(5);"),
    ("ratio", "clk.tick(6);"),
    ("step", "const double ir = rsq1(nd2);"),
    ("add", "if (t2 <= t1) {"),
    ("add_colq", "switch (q & (NL - 1)) {"),
    ("add_householder", "nw[r] = -beta"),
    ("add_tail", "the reflection maps e_q"),
    ("drop", "DROP active position k"),
    ("drop_givens", "for (int j = k; j < q - 1; ++j) {"),
    ("drop_rotate_D", "Tv[l * NL + q - 1] = 0.0;"),
    ("drop_tail", "--q;"),
    ("loop_tail", "clk.tick(9);"),
    ("output", "clk.tick(10);"),
]
COLUMN_SECTIONS = ("slack_product", "back_subst", "add_householder", "drop_rotate_D")


# ------------------------------------------------------------------ replay
def traces(count, family, seed=20261015):
    import oracle
    from gi_select_sim import gi
    H, f, A, b = oracle.family_generate(16, count, seed, family=family, shift=1.0, box=10.0)
    out = []
    for i in range(count):
        tr = []
        gi(H[i], f[i], A[i], b[i], "proj", trace=tr)
        out.append(tr)
    return out


def replay(trs, rows=4):
    """Lockstep waves of `rows` consecutive QPs -> per-trip records and their averages per wave."""
    waves = len(trs) // rows
    trips = []
    for w in range(waves):
        grp = trs[w * rows:(w + 1) * rows]
        fin_q = []
        for t in grp:
            fin_q.append(0 if not t else t[-1][0] + (1 if t[-1][1] == "add" else -1))
        T = max(len(t) for t in grp) + 1  # every row's last trip is the selection that finds nothing
        for k in range(T):
            working = [(t[k], r) for r, t in enumerate(grp) if k < len(t)]
            selecting = [r for r, t in enumerate(grp)
                         if k <= len(t) and (k == 0 or k == len(t) or t[k - 1][1] == "add")]
            # q as the cross-row readlanes see it: a row that has left keeps its final q
            stale = [fin_q[r] for r, t in enumerate(grp) if k >= len(t)]
            qs = [s[0] for s, _ in working]
            adds = [s for s, _ in working if s[1] == "add"]
            drops = [s for s, _ in working if s[1] == "drop"]
            rec = {"wave": w, "work": bool(working), "select": bool(selecting)}
            if working:
                rec.update(qmax=min(max(qs + stale), NL), qmin=min(qs), qmin_all=min(qs + stale),
                           qmax_work=max(qs), uniform=len(set(qs)) == 1, qs=sorted(set(qs)),
                           add=bool(adds), drop=bool(drops), add_distinct=len({s[0] for s in adds}),
                           givens=max([s[0] - 1 - s[2] for s in drops] + [0]),
                           drop_cols=sorted({j for s in drops for j in range(s[2], s[0] - 1)}))
            trips.append(rec)
    work = [t for t in trips if t["work"]]
    per = lambda n: n / waves  # noqa: E731
    its = np.array([len(t) for t in trs[:waves * rows]])
    stats = {
        "qps": waves * rows, "waves": waves,
        "iterations_per_qp": float(its.mean()),
        "trips_per_wave": per(len(trips)),
        "work_trips_per_wave": per(len(work)),
        "select_trips_per_wave": per(sum(t["select"] for t in trips)),
        "add_trips_per_wave": per(sum(t["add"] for t in work)),
        "drop_trips_per_wave": per(sum(t["drop"] for t in work)),
        "work_trips_with_drop": float(np.mean([t["drop"] for t in work])),
        "work_trips_q_uniform": float(np.mean([t["uniform"] for t in work])),
        "mean_qmin": float(np.mean([t["qmin"] for t in work])),
        "mean_qmax_working_rows": float(np.mean([t["qmax_work"] for t in work])),
        "mean_qmax_with_finished_rows": float(np.mean([t["qmax"] for t in work])),
        "mean_qmin_with_finished_rows": float(np.mean([t["qmin_all"] for t in work])),
        "mean_qmin_on_add_trips": float(np.mean([t["qmin"] for t in work if t["add"]])),
        "givens_steps_per_wave": per(sum(t["givens"] for t in work)),
        "add_distinct_q_per_add_trip": float(np.mean([t["add_distinct"] for t in work if t["add"]])),
    }
    return trips, stats


def section_execs(trips, waves, head):
    """Executions per wave of every section; for the column-unrolled ones per column J.
    head: the listing guards the columns below qmin in the two products."""
    work = [t for t in trips if t["work"]]
    n = lambda it: sum(1 for _ in it) / waves  # noqa: E731
    adds = [t for t in work if t["add"]]
    drops = [t for t in work if t["drop"]]
    ex = {
        "setup": 1.0, "output": 1.0,
        "loop_head": n(trips), "select": n(t for t in trips if t["select"]),
        "exchange": n(work), "norm_d2": n(work), "step": n(work), "loop_tail": n(work),
        "slack_product": n(work), "back_subst": n(work),
        "ratio": n(t for t in work if t["qmax"] > 0),
        "add": n(adds), "add_householder": n(adds), "add_tail": n(adds),
        "add_colq": sum(t["add_distinct"] for t in adds) / waves / NL,  # one case block per distinct q
        "drop": n(drops), "drop_tail": n(drops), "drop_rotate_D": n(drops),
        "drop_givens": sum(t["givens"] for t in drops) / waves,
    }
    col = {
        "back_subst": [n(t for t in work if t["qmax"] > J) for J in range(NL)],
        "drop_rotate_D": [n(t for t in drops if J in t["drop_cols"]) for J in range(NL)],
    }
    if head:
        col["slack_product"] = [n(t for t in work if t["qmin"] <= J) for J in range(NL)]
        col["add_householder"] = [n(t for t in adds if t["qmin"] <= J) for J in range(NL)]
    return ex, col


# ------------------------------------------------------------------ listing
def make_listing(source, out):
    inc = os.path.join(ROOT, "include")
    csrc = os.path.join(ROOT, "embedded-qp-solver_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++20", "-O3", "--offload-arch=gfx950", "-fPIC",
           f"-I{inc}", f"-I{inc}/compat", f"-I{csrc}", "-Wno-unused-function", "-mllvm", "-disable-machine-licm",
           "-gline-tables-only", "-x", "hip", source, "--cuda-device-only", "-S", "-o", out]
    subprocess.run(cmd, check=True)


def source_sections(source):
    """[(first line, section)] and the line range of gi_group."""
    lines = open(source).read().split("\n")
    start = next(i for i, l in enumerate(lines) if "void gi_group(" in l) + 1
    end = next(i for i, l in enumerate(lines) if "clk.flush(dbg);" in l) + 1
    marks, at = [], start - 1
    for name, text in ANCHORS:
        at = next(i for i in range(at, len(lines)) if text in lines[i])
        marks.append((at + 1, name))
    return marks, (start, end)


def op_class(op, text):
    c = {}
    if op.startswith("v_"):
        if op.startswith(("v_fma_f64", "v_fmac_f64")):
            c["FMA_F64"] = 1
        elif op.startswith("v_mul_f64"):
            c["MUL_F64"] = 1
        elif op.startswith(("v_add_f64", "v_min_f64", "v_max_f64")):  # min / max issue like an add
            c["ADD_F64"] = 1
        elif op.startswith(("v_rcp_f64", "v_rsq_f64", "v_sqrt_f64")):
            c["TRANS_F64"] = 1
        else:
            c["B32"] = 1
        c["VALU"] = 1
        if "dpp" in op or "row_" in text or "quad_perm" in text:
            c["DPP"] = 1
        if op.startswith("v_cndmask"):
            c["CNDMASK"] = 1
        # 64-bit address arithmetic on the VALU: shifted adds, carry pairs, the sign
        # extension in front of them
        if op.startswith(("v_lshl_add_u64", "v_add_co_u32", "v_addc_co_u32", "v_ashrrev_i32", "v_ashrrev_i64",
                          "v_lshlrev_b64", "v_mad_u64_u32", "v_mad_i64_i32")):
            c["ADDR64"] = 1
        if op.startswith(("v_readlane", "v_readfirstlane")):
            c["READLANE"] = 1
    elif op.startswith("s_"):
        c["SALU"] = 1
    elif op.startswith("ds_"):
        c["LDS"] = 1
    elif op.startswith(("global_", "buffer_", "scratch_", "flat_")):
        c["VMEM"] = 1
    return c


def parse_listing(path, pat, source_name, marks, rng):
    """Blocks of the kernel: label, instructions as (section, class dict, broadcast lane or None)."""
    L = open(path).read().split("\n")
    s = next(i for i, l in enumerate(L) if re.match(r"^" + pat + r"\S*:", l))
    e = next(i for i in range(s, len(L)) if L[i].startswith(".Lfunc_end"))
    base = os.path.basename(source_name)
    frame = re.compile(r"([\w./+-]+):(\d+):\d+")

    def section_of(line):
        sec = "setup"
        for first, name in marks:
            if line >= first:
                sec = name
        return sec

    blocks, cur, sec, seen_loop = [], None, "setup", False
    for l in L[s:e]:
        t = l.strip()
        if re.match(r"^\.LBB[\w$]*:", t) or cur is None:
            # the listing tags every block of the trip loop ("in Loop", "Loop Header", "Parent Loop");
            # a block outside it runs once per wave whatever line its instructions carry (the
            # initial values of the loop's registers carry the `while` line)
            in_loop = "Loop" in t
            seen_loop = seen_loop or in_loop
            cur = {"block": t.split(":")[0][:24], "ins": [], "once": None if in_loop else
                   ("output" if seen_loop else "setup")}
            blocks.append(cur)
            if re.match(r"^[.\w$]+:", t):
                continue
        if t.startswith(".loc"):
            # outermost frame inside gi_group (the chain runs from the innermost frame outwards)
            fr = [(f, int(n)) for f, n in frame.findall(t.split(";", 1)[1])] if ";" in t else []
            inside = [n for f, n in fr if os.path.basename(f) == base and rng[0] <= n <= rng[1]]
            if inside:
                sec = section_of(inside[-1])
            continue
        if not t or t[0] in ".;" or re.match(r"^[.\w$]+:", t):
            continue
        op = t.split()[0]
        m = re.search(r"row_newbcast:(\d+)", t)
        cur["ins"].append((cur["once"] or sec, op_class(op, t), int(m.group(1)) if m else None, op))
    return [b for b in blocks if b["ins"]]


def account(blocks, ex, col):
    """-> per-block rows, per-section totals, totals (all per wave)."""
    rows = []
    sections = collections.defaultdict(lambda: collections.Counter())
    static = collections.defaultdict(lambda: collections.Counter())
    for b in blocks:
        secs = collections.Counter(i[0] for i in b["ins"])
        main = secs.most_common(1)[0][0]
        lanes = {i[2] for i in b["ins"] if i[2] is not None and i[0] in COLUMN_SECTIONS}
        column = lanes.pop() if len(lanes) == 1 and main in col else None
        per = collections.Counter()
        for sec, cls, _, _ in b["ins"]:
            n = col[sec][column] if (column is not None and sec in col) else ex[sec]
            for k in cls:
                per[k] += n
                sections[sec][k] += n
                static[sec][k] += 1
        # (blocks that only wait or branch once per wave add nothing to the table)
        if any(v >= 0.05 for v in per.values()):
            rows.append({"block": b["block"], "section": main, "column": column,
                         "execs_per_wave": round(col[main][column] if column is not None else ex[main], 3),
                         "per_wave": {k: round(v, 1) for k, v in per.items()}})
    tot = collections.Counter()
    for c in sections.values():
        tot.update(c)
    return rows, sections, static, tot


def compact_json(res):
    """One line per top-level key, per section and per block: the table stays readable as a diff."""
    one = lambda v: json.dumps(v, separators=(", ", ": "))  # noqa: E731
    out = []
    for k, v in res.items():
        if k == "sections":
            body = ",\n".join(f"  {json.dumps(s)}: {one(x)}" for s, x in v.items())
            out.append(f' "{k}": {{\n{body}\n }}')
        elif k == "blocks":
            out.append(f' "{k}": [\n' + ",\n".join("  " + one(x) for x in v) + "\n ]")
        else:
            out.append(f' "{k}": {one(v)}')
    return "{\n" + ",\n".join(out) + "\n}"


def issue_cycles(c):
    return sum(c.get(k, 0.0) * v for k, v in VALU_COST.items())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--source", default=os.path.join(ROOT, "embedded-qp-solver_amd", "csrc", "qpb_gi.hip"))
    ap.add_argument("--listing", help="a listing of --source made with -gline-tables-only (default: compile one)")
    ap.add_argument("--kernel", default=FLAGSHIP)
    ap.add_argument("--family", default="box")
    ap.add_argument("--count", type=int, default=2000)
    ap.add_argument("--pmc-valu", type=float, help="SQ_INSTS_VALU per wave of this kernel and family (calibration)")
    ap.add_argument("--label", default="")
    ap.add_argument("--out")
    a = ap.parse_args()

    marks, rng = source_sections(a.source)
    with tempfile.TemporaryDirectory() as tmp:
        listing = a.listing
        if not listing:
            listing = os.path.join(tmp, "qpb_gi.s")
            make_listing(a.source, listing)
        blocks = parse_listing(listing, a.kernel, a.source, marks, rng)
    head = "wave_min4(" in open(a.source).read()  # the dead-column guards are in this source
    trips, stats = replay(traces(a.count, a.family))
    ex, col = section_execs(trips, stats["waves"], head)
    rows, sections, static, tot = account(blocks, ex, col)

    cyc = issue_cycles(tot)
    loop = collections.Counter()
    for sec, c in sections.items():
        if sec not in ("setup", "output"):
            loop.update(c)
    f64 = ("FMA_F64", "MUL_F64", "ADD_F64", "TRANS_F64")
    non64 = sorted(((sec, c["B32"], c["B32"] * VALU_COST["B32"]) for sec, c in sections.items()), key=lambda x: -x[1])
    res = {
        "label": a.label, "kernel": a.kernel, "family": a.family, "dead_column_guards": head,
        "replay": stats,
        "per_wave": {k: round(v, 1) for k, v in tot.items()},
        "issue_cycles_per_wave": round(cyc, 1),
        "loop_per_wave": {k: round(v, 1) for k, v in loop.items()},
        "non_fp64_share_of_valu": {"kernel": tot["B32"] / tot["VALU"], "loop": loop["B32"] / loop["VALU"]},
        "non_fp64_share_of_issue_cycles": {"kernel": tot["B32"] * VALU_COST["B32"] / cyc,
                                           "loop": loop["B32"] * VALU_COST["B32"] / issue_cycles(loop)},
        "sections": {sec: {"execs_per_wave": round(ex[sec], 3),
                           "static": dict(static[sec]),
                           "per_wave": {k: round(v, 1) for k, v in c.items()},
                           "issue_cycles_per_wave": round(issue_cycles(c), 1),
                           "share_of_issue_cycles": round(issue_cycles(c) / cyc, 4)}
                     for sec, c in sections.items()},
        "column_execs_per_wave": {k: [round(x, 3) for x in v] for k, v in col.items()},
        "top_non_fp64": [{"section": s, "b32_per_wave": round(n, 1), "share_of_issue_cycles": round(cy / cyc, 4)}
                         for s, n, cy in non64[:5]],
        "blocks": rows,
    }
    if a.pmc_valu:
        res["calibration"] = {"pmc_valu_per_wave": a.pmc_valu, "table_valu_per_wave": round(tot["VALU"], 1),
                              "ratio": tot["VALU"] / a.pmc_valu, "within_5_percent": abs(tot["VALU"] / a.pmc_valu - 1) <= 0.05}
    text = compact_json(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    brief = {k: res[k] for k in ("label", "family", "replay", "per_wave", "issue_cycles_per_wave",
                                 "non_fp64_share_of_valu", "non_fp64_share_of_issue_cycles", "top_non_fp64")}
    brief["sections"] = {s: (v["execs_per_wave"], v["per_wave"].get("VALU", 0), v["share_of_issue_cycles"])
                         for s, v in res["sections"].items()}
    if "calibration" in res:
        brief["calibration"] = res["calibration"]
    print(json.dumps(brief, indent=1))


if __name__ == "__main__":
    main()
