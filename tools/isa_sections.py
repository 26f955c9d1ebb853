#!/usr/bin/env python3
"""Vector-instruction counts of one k_render instantiation, section by section (offline: hipcc cross-compiles, no GPU).

    python tools/isa_sections.py                       # k_render<false, 64, true, false>, the headline kernel (lean, PLAIN form;
                                                       # its generic form is k_render<false, 0, true, false>)
    python tools/isa_sections.py "k_render<false, 4, true, false>" [-DPRT_X=1 ...] [--json] [--list] [--show=SECTION] [--opcodes]
    python tools/isa_sections.py --csrc=DIR [--asm=FILE]   # another checkout's csrc/ (and an assembly already made from it)

The kernel file is compiled to assembly with line tables (-gline-tables-only: the instruction stream is the product's, each
instruction carries the chain of inlined source lines it came from) and every instruction of the named kernel is booked to
the section whose source it was inlined from:

  node visit       Trav::inner_step, Trav::box4
  round control    Trav::round and the wave loop of k_render around the steps (the ballots, counts and thresholds)
  leaf entry/exit  Trav::leaf_step and test_leaf / test_leaf_pp outside their loop
  leaf iteration   the loop of test_leaf / test_leaf_pp with tri_test / tri_test_ord, per copy of the loop body
  chain step       the in-loop chain step of k_render
  set-up           Trav::start / slab_axis where they kept their lines (a copy the compiler hoisted carries none and is booked
                   to whatever precedes it: `hoisted` or `pass`); the number of sites is counted from the three v_rcp_f32 of each
  hoisted          instructions booked to a line of k_render's wave loop that sit outside it (loop depth below 2 in the
                   compiler's block comments): what the compiler moved out of the loop, e.g. the chain step's set-up, which
                   then carries no line of Trav::start.  Hoisted code that kept its own line is booked to that line's section.
  pass             everything else inside k_render's pass loop
  prologue         before the pass loop

It counts instruction classes, nothing else: VALU (v_*), vector memory (global_ / flat_ / scratch_ / buffer_) and LDS (ds_)
make up "vector"; scalar instructions are listed beside them.  `moves` are the register copies among the VALU instructions
(v_mov_b32 + v_mov_b64: what the register allocator adds at block joins, and constants).  --opcodes prints, below the table,
every section's instructions by opcode, most frequent first (with --json: under "opcodes").  Registers, spills and occupancy
are read from the kernel's metadata in the same assembly.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pooraytracer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-Wno-unused-function", "-fno-gpu-rdc"]  # build.py's CFLAGS
SECTIONS = ("node visit", "round control", "leaf entry/exit", "leaf iteration", "chain step", "set-up", "hoisted", "pass", "prologue")
MOVES = ("v_mov_b32", "v_mov_b64")
WAVE_LOOP = ("node visit", "round control", "leaf entry/exit", "leaf iteration", "chain step")  # sections that live at loop depth >= 2


def function_ranges(path):
    """{name: [(first line, last line), ...]} of the PRT_DEV functions of a source (a function ends where the next one,
    or the next struct / template / section comment at its indentation or less, begins)."""
    lines = open(path).read().split("\n")
    starts = []
    for i, l in enumerate(lines, 1):
        m = re.match(r"\s*PRT_DEV\s+[\w:<>&\*\s]+?\b(\w+)\s*\(", l)
        if m:
            starts.append((i, m.group(1)))
    out = {}
    for k, (ln, name) in enumerate(starts):
        end = starts[k + 1][0] - 1 if k + 1 < len(starts) else len(lines)
        for j in range(ln + 1, end + 1):  # stop at the next declaration that is not inside this function
            if re.match(r"(\s*)(template\s*<|struct\s|// -{10,})", lines[j - 1]) and not lines[j - 1].startswith(" " * 8):
                end = j - 1
                break
        out.setdefault(name, []).append((ln, end))
    return out, lines


def loop_line(lines, rng):
    """First line of the triangle loop inside a test_leaf range."""
    for j in range(rng[0], rng[1] + 1):
        if re.match(r"\s*for\s*\(", lines[j - 1]):
            return j
    return rng[0]


class Classifier:
    def __init__(self):
        dev, dl = function_ranges(os.path.join(CSRC, "prt_device.h"))
        self.dev = dev
        self.leaf_loops = [(loop_line(dl, r), r[1]) for n in ("test_leaf", "test_leaf_pp") for r in dev.get(n, [])]
        k = open(os.path.join(CSRC, "prt_kernels.hip")).read().split("\n")
        self.pass_begin = next(i for i, l in enumerate(k, 1) if re.match(r"\s*for \(;;\) \{", l) and "n_refills" in k[i])
        self.loop_begin = next(i for i, l in enumerate(k, 1) if "traversal steps until enough lanes have finished" in l)
        self.kernel_end = next(i for i, l in enumerate(k, 1) if i > self.loop_begin and "wave_sum((unsigned long long)wc.nodes)" in l)
        self.chain = []
        b = None
        for i in range(self.loop_begin, self.kernel_end):
            if "PROF_MARK(0);" in k[i - 1] and b is None:
                b = i
            if "PROF_MARK(5);" in k[i - 1] and b is not None:
                self.chain.append((b, i))
                b = None

    def _in(self, names, line):
        return any(a <= line <= b for n in names for a, b in self.dev.get(n, []))

    def section(self, stack):
        """`stack`: [(file basename, line), ...] innermost first."""
        dev = [l for f, l in stack if f == "prt_device.h"]
        ker = [l for f, l in stack if f == "prt_kernels.hip"]
        if ker and ker[-1] < self.pass_begin:
            return "prologue"  # (Trav::init before the pass loop is not a set-up site of a path vertex)
        if any(self._in(("inner_step", "box4"), l) for l in dev):
            return "node visit"
        if any(self._in(("start", "slab_axis", "init"), l) for l in dev):
            return "set-up"
        if any(self._in(("tri_test", "tri_test_ord"), l) for l in dev) or any(a <= l <= b for l in dev for a, b in self.leaf_loops):
            return "leaf iteration"
        if any(self._in(("leaf_step", "test_leaf", "test_leaf_pp"), l) for l in dev):
            return "leaf entry/exit"
        if any(self._in(("round",), l) for l in dev):
            return "round control"
        if ker:
            l = ker[-1]  # the outermost frame: where in k_render
            if any(a <= l <= b for a, b in self.chain):
                return "chain step"
            if self.loop_begin <= l < self.kernel_end:
                return "round control"
            if l >= self.pass_begin:
                return "pass"
            return "prologue"
        return None


def kind(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith(("global_", "flat_", "scratch_", "buffer_")):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("s_"):
        return "scalar"
    return None


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    out = {}
    for n, d in zip(names, p.stdout.split("\n")):
        d = d.replace("(anonymous namespace)::", "").replace("void ", "")
        out[n] = re.sub(r"\(.*", "", d)
    return out


def assembly(extra, given=None):
    """Lines of the kernel file's device assembly with line tables (`given`: a file made earlier by the same command)."""
    if given:
        return open(given).read().split("\n")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "k.s")
        cmd = [HIPCC, "-S", "--cuda-device-only", "-gline-tables-only"] + FLAGS + extra + ["-o", asm, os.path.join(CSRC, "prt_kernels.hip")]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode:
            sys.stderr.write(p.stderr)
            raise SystemExit(p.returncode)
        return open(asm).read().split("\n")


def main():
    global CSRC
    args = sys.argv[1:]
    CSRC = next((a.split("=", 1)[1] for a in args if a.startswith("--csrc=")), CSRC)  # the sources of another checkout
    extra = [a for a in args if a.startswith("-D")]
    want = next((a for a in args if not a.startswith("-")), "k_render<false, 64, true, false>")
    text = assembly(extra, next((a.split("=", 1)[1] for a in args if a.startswith("--asm=")), None))
    funcs = [m.group(1) for l in text for m in [re.match(r"\s*\.type\s+(\S+),@function", l)] if m]
    names = demangle(funcs)
    if "--list" in args:
        print("\n".join(sorted(v for v in names.values() if v.startswith("k_"))))
        return
    sym = next((s for s, d in names.items() if d == want), None)
    if sym is None:
        raise SystemExit(f"no kernel named {want!r}; --list shows the names")
    begin = text.index(next(l for l in text if l.startswith(sym + ":")))
    end = next(i for i in range(begin, len(text)) if text[i].startswith(".Lfunc_end"))
    C = Classifier()
    counts = {s: {"valu": 0, "vmem": 0, "lds": 0, "scalar": 0} for s in SECTIONS}
    marks = {s: {} for s in SECTIONS}
    opcodes = {s: {} for s in SECTIONS}
    cur = "prologue"
    show = next((a.split("=", 1)[1] for a in args if a.startswith("--show=")), None)  # print that section's instructions
    depth, in_head, from_device = 0, False, False
    for l in text[begin:end]:
        if re.match(r"(\.LBB\d+_\d+:|; %bb\.\d+:)", l):  # a new block: its loop depth is in the comment (a header's: the lines below)
            d = re.findall(r"Depth[= ](\d+)", l)
            depth, in_head = (max(map(int, d)) if d else 0), True
            continue
        if in_head and re.match(r"\s+;", l):
            d = re.findall(r"Depth[= ](\d+)", l)
            depth = max([depth] + list(map(int, d)))
            continue
        m = re.match(r"\s*\.loc\s+\d+\s+(\d+)\s+\d+.*?;\s*(\S.*)$", l)
        if m:
            if int(m.group(1)) != 0:  # (line 0: compiler-generated, stays with the section before it)
                stack = [(os.path.basename(f), int(n)) for f, n in re.findall(r"([^\s\[\]@]+):(\d+):\d+", m.group(2))]
                cur = C.section(stack) or cur
                from_device = any(f == "prt_device.h" for f, _ in stack)
            continue
        m = re.match(r"\s+([a-z][a-z0-9_]+)(\s|$)", l)
        if not m or l.lstrip().startswith((".", ";")):
            continue
        k = kind(m.group(1))
        if k is None:
            continue
        in_head = False
        sec = "hoisted" if cur in WAVE_LOOP and depth < 2 and not from_device else cur
        counts[sec][k] += 1
        if show == sec:
            print(l)
        op = re.sub(r"_e(32|64)$", "", m.group(1))
        opcodes[sec][op] = opcodes[sec].get(op, 0) + 1
        if op in ("v_rcp_f32", "v_div_fmas_f64", "v_div_fmas_f32", "v_pk_fma_f32", "v_cvt_f32_u32", "v_alignbit_b32", "v_mov_b64", "v_max_f64"):
            marks[sec][op] = marks[sec].get(op, 0) + 1
    entry = next((e for e in re.split(r"\n  - (?=\.agpr_count:)", "\n".join(text)) if re.search(r"\.name:\s+" + re.escape(sym) + r"\s", e)), "")
    meta = {k: int(v) for k, v in re.findall(r"\.(agpr_count|vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s*(\d+)", entry)}
    occ = re.search(r"; Occupancy:\s*(\d+)", "\n".join(text[end:end + 80]))
    vec = {s: c["valu"] + c["vmem"] + c["lds"] for s, c in counts.items()}
    moves = {s: sum(opcodes[s].get(op, 0) for op in MOVES) for s in SECTIONS}
    by_count = {s: sorted(opcodes[s].items(), key=lambda kv: (-kv[1], kv[0])) for s in SECTIONS}
    copies = max(1, marks["leaf iteration"].get("v_div_fmas_f64", 0) + marks["leaf iteration"].get("v_div_fmas_f32", 0))
    sites = sum(marks[x].get("v_rcp_f32", 0) for x in SECTIONS if x != "prologue") // 3
    report = {
        "kernel": want, "flags": extra,
        "vector": vec, "scalar": {s: c["scalar"] for s, c in counts.items()}, "detail": counts, "moves": moves,
        "leaf_loop_copies": copies, "leaf_iteration_vector": vec["leaf iteration"] / copies,
        "setup_sites": sites, "pass_static_vector": vec["pass"] + vec["set-up"] + vec["hoisted"],
        "total_vector": sum(vec.values()),
        "v_mov_b64_in_leaf_iteration": marks["leaf iteration"].get("v_mov_b64", 0),
        "v_max_f64_in_leaf_iteration": marks["leaf iteration"].get("v_max_f64", 0),
        "vgprs": meta.get("vgpr_count"), "agprs": meta.get("agpr_count"), "sgprs": meta.get("sgpr_count"),
        "scratch_bytes_per_lane": meta.get("private_segment_fixed_size"),
        "vgpr_spill": meta.get("vgpr_spill_count"), "sgpr_spill": meta.get("sgpr_spill_count"),
        "occupancy": int(occ.group(1)) if occ else None,
    }
    if "--opcodes" in args:
        report["opcodes"] = {s: dict(by_count[s]) for s in SECTIONS}
    if "--json" in args:
        print(json.dumps(report, indent=1))
        return
    print(f"{want}" + (f"  [{' '.join(extra)}]" if extra else ""))
    print(f"{'section':18s} {'vector':>7s} {'VALU':>6s} {'VMEM':>5s} {'LDS':>4s} {'moves':>6s} {'scalar':>7s}")
    for s in SECTIONS:
        c = counts[s]
        note = ""
        if s == "leaf iteration":
            note = f"   {copies} cop{'ies' if copies > 1 else 'y'} of the loop body: {vec[s] / copies:.1f} per iteration"
        if s == "set-up":
            note = f"   {sites} site{'s' if sites != 1 else ''} in the whole pass (v_rcp_f32 / 3, wherever they are booked)"
        print(f"{s:18s} {vec[s]:7d} {c['valu']:6d} {c['vmem']:5d} {c['lds']:4d} {moves[s]:6d} {c['scalar']:7d}{note}")
    print(f"{'whole kernel':18s} {sum(vec.values()):7d}")
    print(f"VGPR {report['vgprs']} AGPR {report['agprs']} SGPR {report['sgprs']} spilled VGPR {report['vgpr_spill']} SGPR {report['sgpr_spill']} "
          f"scratch {report['scratch_bytes_per_lane']} B/lane occupancy {report['occupancy']}")
    if "--opcodes" in args:
        for s in SECTIONS:
            if by_count[s]:
                print(f"\n{s}: " + "  ".join(f"{op} {n}" for op, n in by_count[s]))


if __name__ == "__main__":
    main()
