"""The packed SW fill with column classes of period C / 2 (agx_sw_pk2w_kernel.hip) as the compiler built
it: the DNA-coded quad loop at 38 columns per lane -- the headline's, in sw_fill_pk2w<38> and in the one-launch kernel
sw_fill_pk2w_any -- is disassembled from libagx.so and held to its instruction budget, in the style of
tests/test_sw_step_budget_cpu.py:
  * the loop is the one with 4 C v_perm_b32, a load and exactly 4 (C + 2) v_sub_u32 -- per step one per column (z = H - open), ONE
    class wrap and one arrival, where the period of four has nine wraps a step (192);
  * without the corner test it issues at most MAX_VALU vector instructions and MAX_NOP s_nop (1075 and 6 at period four);
  * every class's own kernel and the one-launch kernel: at most 256 VGPRs, no AGPRs, no scratch;
  * the row-load discipline of tests/test_sw_isa_cpu.py holds in the new kernels too."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from tests import sw_period_ref as pref
from tests.test_sw_isa_cpu import LIB, MAX_HEAD_WAITS, MIN_VALU, _distance_to_wait, _loading_loops, _loops, _op, _path_to, _tool, _vmcnt, built  # noqa: F401

C = 38
MAX_VALU = 1054
MAX_NOP = 0
ARGS = "E8SwParamsPKjPK8SwGroup2PK6SwWavejPi"
KERNELS = {
    "sw_fill_pk2w<38>": "_ZN12_GLOBAL__N_112sw_fill_pk2wILi38EEEv" + ARGS[1:],
    "sw_fill_pk2w_any": "_ZN12_GLOBAL__N_116sw_fill_pk2w_any" + ARGS,
}


def disassemble(lib, want):
    """{mangled kernel name: [instruction text or 'LABEL name', ...]} for the kernels `want` names."""
    objdump = os.path.join(_tool().LLVM, "llvm-objdump")
    want = set(want)
    out = {}
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(lib, os.path.join(d, "lib.so"))
        subprocess.run([objdump, "--offloading", "lib.so"], cwd=d, capture_output=True, check=True)
        for f in sorted(os.listdir(d)):
            if "amdgcn" not in f:
                continue
            syms = subprocess.run([objdump, "-t", os.path.join(d, f)], capture_output=True, text=True, check=True).stdout
            if not any(k in syms for k in want):
                continue
            text = subprocess.run([objdump, "-d", "--no-show-raw-insn", "--symbolize-operands", os.path.join(d, f)],
                                  capture_output=True, text=True, check=True).stdout
            cur = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
                if m:
                    name = m.group(1)
                    if re.match(r"^L\d+$", name):
                        if cur is not None:
                            cur.append("LABEL " + name)
                    else:
                        cur = out.setdefault(name, []) if name in want else None
                elif cur is not None and line.startswith("\t"):
                    ins = line.strip().split(";")[0].split("//")[0].strip()
                    if ins:
                        cur.append(ins)
    missing = want - set(out)
    assert not missing, "kernels not found in libagx.so: %s" % sorted(missing)
    return out


@pytest.fixture(scope="module")
def disassembly(built):
    return disassemble(built, KERNELS.values())


def _wide_quad_loops(ins):
    out = []
    for lo, hi in _loops(ins):
        body = [_op(ins[j]) for j in range(lo, hi + 1) if not ins[j].startswith("LABEL ")]
        if (body.count("v_perm_b32") == 4 * C and any(op.startswith("global_load") for op in body)
                and body.count("v_sub_u32_e32") + body.count("v_sub_u32") + body.count("v_sub_u32_e64") == 4 * (C + 2)):
            out.append(body)
    return out


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_wide_quad_loop_without_the_corner_test(disassembly, kernel):
    loops = _wide_quad_loops(disassembly[KERNELS[kernel]])
    assert loops, "%s: no DNA-coded quad loop of %d columns with one wrap a step found" % (kernel, C)
    free = [b for b in loops if not any(op.startswith("v_cmp_eq_u32") for op in b)]
    assert free, "%s: every DNA-coded quad loop tests for the corner" % kernel
    for body in free:
        valu = sum(op.startswith("v_") for op in body)
        nop = sum(op == "s_nop" for op in body)
        print("%s: %d VALU, %d s_nop, %d v_pk_max_u16, %d v_pk_maximum3_f16, %d scalar adds a quad" % (
            kernel, valu, nop, sum(op.startswith("v_pk_max_u16") for op in body), sum(op.startswith("v_pk_maximum3_f16") for op in body),
            sum(op.startswith(("s_add_i32", "s_add_u32")) for op in body)))
        assert valu <= MAX_VALU, "%s: %d VALU instructions a quad (budget %d)" % (kernel, valu, MAX_VALU)
        assert nop <= MAX_NOP, "%s: %d s_nop a quad (budget %d)" % (kernel, nop, MAX_NOP)


def test_every_wide_class_fits_two_waves_per_simd(built):
    """Each class from 14 columns on has a wide build (sw_period_ref.KEEP_NARROW lists the ones that must not), and each of
    them, like the one-launch kernel that is allocated for the widest, stays within 256 VGPRs without AGPRs or scratch."""
    res = _tool().kernel_resources(built)
    names = ["sw_fill_pk2w<%d>" % c for c in pref.PACKED_CLASSES if pref.period(c) > pref.NARROW] + ["sw_fill_pk2w_any"]
    assert len(names) > 1
    for k in names:
        assert k in res, (k, sorted(n for n in res if "pk2w" in n))
        r = res[k]
        assert r["vgpr"] <= 256 and r["agpr"] == 0 and r["scratch"] == 0, (k, r)
    for c in pref.PACKED_CLASSES:
        if pref.period(c) == pref.NARROW:
            assert "sw_fill_pk2w<%d>" % c not in res, c


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_row_loads_stay_in_flight(disassembly, kernel):
    ins = disassembly[KERNELS[kernel]]
    loops = _loading_loops(ins)
    assert loops, "no loop of %s loads" % kernel
    for lo, hi in loops:
        for i in range(lo, hi + 1):
            if _op(ins[i]).startswith("global_load"):
                d = _distance_to_wait(ins, lo, hi, i)
                assert d is None or d >= MIN_VALU, "%s: %r at %d is waited for after %d VALU instructions (< %d)" % (
                    kernel, ins[i], i, d, MIN_VALU)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_wave_head_waits_at_most_twice(disassembly, kernel):
    ins = disassembly[KERNELS[kernel]]
    for lo, _ in _loading_loops(ins):
        outstanding, waits = 0, []
        for j in _path_to(ins, lo):
            n = _vmcnt(ins[j])
            if n is not None and outstanding > n:
                waits.append(ins[j])
                outstanding = n
            elif _op(ins[j]).startswith(("global_", "buffer_", "flat_", "scratch_")):
                outstanding += 1
        assert len(waits) <= MAX_HEAD_WAITS, "%s: %d vmcnt waits ahead of the loop at %d: %s" % (kernel, len(waits), lo, waits)
