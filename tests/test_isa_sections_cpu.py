"""tools/isa_sections.py books instructions to sections by the source lines they were inlined from.  No compiler here: the
tool's reading of the two source files, and its bookkeeping on a few hand-written lines of assembly with line tables."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("isa_sections", os.path.join(ROOT, "tools", "isa_sections.py"))
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)


def _line_of(path, text, after=0):
    with open(path) as f:
        return next(i for i, l in enumerate(f, 1) if i > after and text in l)


def test_the_tool_finds_its_landmarks_in_the_sources():
    C = T.Classifier()
    for name in ("inner_step", "box4", "start", "slab_axis", "tri_test", "tri_test_ord", "test_leaf", "test_leaf_pp", "leaf_step", "round"):
        assert C.dev.get(name), name
    dev = os.path.join(T.CSRC, "prt_device.h")
    a, b = C.dev["inner_step"][0]
    assert a < _line_of(dev, "PRT_CE(k1, r1, k2, r2)") < b          # the sorting network's macro does not end the function
    assert len(C.leaf_loops) == 2 and all(a < b for a, b in C.leaf_loops)
    assert C.pass_begin < C.loop_begin < C.kernel_end
    assert len(C.chain) == 2 and all(C.loop_begin < a < b < C.kernel_end for a, b in C.chain)  # the diet loop's and the other's


def test_sections_follow_the_inline_chain():
    C = T.Classifier()
    dev, ker = os.path.join(T.CSRC, "prt_device.h"), os.path.join(T.CSRC, "prt_kernels.hip")
    visit = _line_of(dev, "const uint4 bx = np[0]")
    plane = _line_of(dev, "real denom = dot_yxz")
    pop = _line_of(dev, "cur = (int32_t)stk[sp * 64];", after=C.dev["leaf_step"][0][0])
    slab = _line_of(dev, "float id = __builtin_amdgcn_rcpf(df);")
    in_loop = C.loop_begin + 5
    assert C.section([("prt_device.h", visit), ("prt_kernels.hip", in_loop)]) == "node visit"
    assert C.section([("prt_device.h", 54), ("prt_device.h", plane), ("prt_kernels.hip", in_loop)]) == "leaf iteration"
    assert C.section([("prt_device.h", pop), ("prt_kernels.hip", in_loop)]) == "leaf entry/exit"
    assert C.section([("prt_device.h", slab), ("prt_kernels.hip", C.chain[0][0] + 3)]) == "set-up"
    assert C.section([("prt_kernels.hip", C.chain[0][0] + 1)]) == "chain step"
    assert C.section([("prt_kernels.hip", in_loop)]) == "round control"
    assert C.section([("prt_kernels.hip", C.pass_begin + 10)]) == "pass"
    assert C.section([("prt_device.h", slab), ("prt_kernels.hip", _line_of(ker, "tr.init(S, mk3(0, 0, 0), rd"))]) == "prologue"
    assert T.kind("v_pk_fma_f32") == "valu" and T.kind("global_load_dwordx4") == "vmem" and T.kind("ds_read_b32") == "lds"
    assert T.kind("s_bcnt1_i32_b64") == "scalar" and T.kind("foo") is None
