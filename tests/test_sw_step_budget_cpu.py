"""What a quad of steps of the packed SW fill issues besides its cells (agx_sw_pk2_kernel.hip):
the DNA-coded quad loop at 38 columns per lane -- the headline's, in sw_fill_pk2<38, 4> and in the one-launch kernel
sw_fill_pk2_any<4> -- is disassembled from libagx.so and held to its instruction budget:
  * a copy of the loop without the corner test (no v_cmp_eq_u32) runs the quads before a wave's first corner step;
  * that loop issues at most MAX_VALU vector instructions (1107 before the corner test left it, the maxima were kept
    per offset and the first column took its class offset off once) and at most MAX_NOP s_nop;
  * two waves per SIMD: at most 256 VGPRs, no scratch."""
import pytest

from tests.test_sw_isa_cpu import KERNELS, _loops, _op, _tool, built, disassembly  # noqa: F401 (fixtures)

C = 38
MAX_VALU = 1080
MAX_NOP = 6


def _quad_loops(ins):
    """Loops that load (the row stream) and hold the DNA-coded cells of C columns: 4 C v_perm_b32 a quad."""
    out = []
    for lo, hi in _loops(ins):
        body = [_op(ins[j]) for j in range(lo, hi + 1) if not ins[j].startswith("LABEL ")]
        if body.count("v_perm_b32") == 4 * C and any(op.startswith("global_load") for op in body):
            out.append(body)
    return out


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_quad_loop_without_the_corner_test(disassembly, kernel):
    loops = _quad_loops(disassembly[KERNELS[kernel]])
    assert loops, "%s: no DNA-coded quad loop of %d columns found" % (kernel, C)
    free = [b for b in loops if not any(op.startswith("v_cmp_eq_u32") for op in b)]
    assert free, "%s: every DNA-coded quad loop tests for the corner" % kernel
    for body in free:
        valu = sum(op.startswith("v_") for op in body)
        nop = sum(op == "s_nop" for op in body)
        assert valu <= MAX_VALU, "%s: %d VALU instructions a quad (budget %d)" % (kernel, valu, MAX_VALU)
        assert nop <= MAX_NOP, "%s: %d s_nop a quad (budget %d)" % (kernel, nop, MAX_NOP)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_registers_within_two_waves_per_simd(built, kernel):
    r = _tool().kernel_resources(built)[kernel]
    assert r["vgpr"] <= 256 and r["agpr"] == 0 and r["scratch"] == 0, r
