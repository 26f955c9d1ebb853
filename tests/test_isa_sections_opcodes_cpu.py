"""tools/isa_sections.py's `moves` column and its --opcodes histogram, on a few hand-written lines of assembly with line
tables (no compiler here: --asm= gives the tool an assembly made earlier; the source lines are looked up in the sources)."""
import json
import os
import sys

from tests.test_isa_sections_cpu import T, _line_of


def _canned(tmp_path):
    """A kernel `k_canned`: three instructions of a node visit in the wave loop (one a register copy), then five of the pass
    (two copies, one of them _e32-suffixed, one scalar), then its end."""
    C = T.Classifier()
    dev = os.path.join(T.CSRC, "prt_device.h")
    visit = _line_of(dev, "const uint4 bx = np[0]")
    in_loop, in_pass = C.loop_begin + 5, C.pass_begin + 10
    text = f"""\t.type\tk_canned,@function
k_canned:
.LBB0_1:                                ; Depth=2
\t.loc\t2 {visit} 9 ; prt_device.h:{visit}:9 @[ prt_kernels.hip:{in_loop}:17 ]
\tglobal_load_dwordx4 v[8:11], v20, s[60:61] offset:48
\tv_mov_b32_e32 v4, v39
\tv_pk_fma_f32 v[2:3], v[4:5], v[6:7], v[8:9]
.LBB0_2:                                ; Depth=1
\t.loc\t1 {in_pass} 5 ; prt_kernels.hip:{in_pass}:5
\tv_mov_b64_e32 v[94:95], v[100:101]
\tv_mov_b32_e32 v5, 0
\tv_add_f64 v[8:9], v[24:25], v[104:105]
\tv_add_f64 v[10:11], v[26:27], v[102:103]
\ts_or_b64 exec, exec, s[10:11]
.Lfunc_end0:
"""
    path = tmp_path / "canned.s"
    path.write_text(text)
    return str(path)


def _run(monkeypatch, capsys, *args):
    monkeypatch.setattr(sys, "argv", ["isa_sections.py", "k_canned", *args])
    T.main()
    return capsys.readouterr().out


def test_moves_are_counted_per_section(tmp_path, monkeypatch, capsys):
    r = json.loads(_run(monkeypatch, capsys, f"--asm={_canned(tmp_path)}", "--json"))
    assert r["vector"]["node visit"] == 3 and r["vector"]["pass"] == 4 and r["scalar"]["pass"] == 1
    assert r["moves"]["node visit"] == 1 and r["moves"]["pass"] == 2
    assert sum(r["moves"].values()) == 3 and "opcodes" not in r
    table = _run(monkeypatch, capsys, f"--asm={_canned(tmp_path)}")
    head, rows = table.split("\n")[1].split(), {l[:18].strip(): l[18:].split() for l in table.split("\n")[2:]}
    col = head.index("moves") - 1  # (the section's name is the first column)
    assert head[col:col + 3] == ["LDS", "moves", "scalar"]
    assert rows["node visit"][:6] == ["3", "2", "1", "0", "1", "0"] and rows["pass"][:6] == ["4", "4", "0", "0", "2", "1"]
    assert rows["leaf iteration"][4] == "0"


def test_the_opcode_histogram(tmp_path, monkeypatch, capsys):
    r = json.loads(_run(monkeypatch, capsys, f"--asm={_canned(tmp_path)}", "--json", "--opcodes"))
    assert r["opcodes"]["node visit"] == {"global_load_dwordx4": 1, "v_mov_b32": 1, "v_pk_fma_f32": 1}
    assert r["opcodes"]["pass"] == {"v_add_f64": 2, "s_or_b64": 1, "v_mov_b32": 1, "v_mov_b64": 1}  # (encoding suffixes dropped)
    assert list(r["opcodes"]["pass"])[0] == "v_add_f64"                                              # most frequent first
    assert all(not r["opcodes"][s] for s in T.SECTIONS if s not in ("node visit", "pass"))
    out = _run(monkeypatch, capsys, f"--asm={_canned(tmp_path)}", "--opcodes")
    assert "\npass: v_add_f64 2  s_or_b64 1  v_mov_b32 1  v_mov_b64 1" in out
    assert "\nnode visit: global_load_dwordx4 1  v_mov_b32 1  v_pk_fma_f32 1" in out
    assert "\nprologue:" not in out and "\nleaf iteration:" not in out
