"""The host's choice between the wide (C / 2) and the narrow (4) period of the packed SW fill's column classes flips exactly
where tests/sw_period_ref.py says it does.

Plan-only batches (no device) are created under the tuning build's AGX_TRACE_CREATE, whose line "class period P of W" names the
period the batch runs (P: W when wide, 4 when narrow) and the largest period W among the classes it launches.  AGX_SW_FORCE_C
pins the columns per lane, and with them W; the batch at the last ll the restated rule still calls wide and the one at ll + 1
are probed, in one child process per scoring and class (the library is chosen when api.py is imported)."""
import json
import os
import re
import subprocess
import sys
import textwrap

import pytest

from tests import sw_period_ref as pref
from tests import sw_range_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = (1, -1, -3, -1)

_CHILD = textwrap.dedent("""
    import json, sys
    sys.path.insert(0, %r)
    import accelerating_genomics_amd.api as agx
    import accelerating_genomics_amd.synth as synth
    assert agx.LIB_PATH.endswith("libagx_tuning.so"), agx.LIB_PATH
    scoring, probes = json.loads(sys.argv[1])
    for k, p in enumerate(probes):
        sys.stderr.write("PROBE %%d\\n" %% k)
        sys.stderr.flush()
        if p[0] == "pair":  # a short pair beside the long one: the rule reads the batch's longest sides, not one pair's
            _, ls, ll = p
            b = synth.sw_from_seqs([b"A" * ls, b"C" * ll, b"A", b"CC"] if k %% 2 else [b"C" * ll, b"A" * ls])
        else:
            _, n, lo, hi, seed = p
            b = synth.sw_pairs(n, lo, hi, seed=seed)
        agx.SwBatch(None, b, tuple(scoring)).close()
    sys.stderr.write("PROBE end\\n")
""") % ROOT


def _trace(scoring, probes, **knobs):
    """-> [(rising, period run, widest period launched)] per probe; (rising, None, None) where no class period is printed."""
    env = dict(os.environ, AGX_TRACE_CREATE="1", **knobs)
    env.pop("AGX_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps([list(scoring), probes])], capture_output=True, timeout=300, env=env)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-2000:]
    parts = re.split(r"^PROBE \w+\n", err, flags=re.M)[1:-1]
    assert len(parts) == len(probes), err[-2000:]
    out = []
    for text in parts:
        rising = re.findall(r"family 2 rising (\d+):", text)
        m = re.findall(r"class period (\d+) of (\d+)\n", text)
        assert len(rising) == 1 and len(m) <= 1, text
        out.append((int(rising[0]),) + ((int(m[0][0]), int(m[0][1])) if m else (None, None)))
    return out


def _pairs(probes):
    return [["pair", ls, ll] for ls, ll in probes]


@pytest.mark.parametrize("scoring,ls,C", [(REF, 150, 38), (REF, 150, 14), (REF, 2560, 40), ((12, -4, -10, -3), 150, 38), ((12, -4, -10, -3), 150, 40),
                                          ((3, -1, -3, -1), 150, 38), ((3, -1, -3, -1), 14, 14), ((4, -1, -30, -5), 40, 40)],
                         ids=lambda v: "_".join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_library_flips_where_the_restated_rule_does(scoring, ls, C):
    P = pref.period(C)
    assert P == C // 2 and ref.variant(scoring, ls, ls) == ("biased", 4)
    L = pref.last_wide_ll(scoring, ls, P)
    Lr = ref.last_rising_ll(scoring, ls)
    assert L is not None and ls < L and L + 1 < Lr, (L, Lr)
    assert pref.wide(scoring, ls, L, P) and not pref.wide(scoring, ls, L + 1, P)
    got = _trace(scoring, _pairs([(ls, ls), (ls, L), (ls, L + 1), (ls, Lr), (ls, Lr + 1)]), AGX_SW_FORCE_C=str(C))
    assert got == [(4, P, P), (4, P, P), (4, 4, P), (4, 4, P), (0, None, None)], (scoring, ls, C, L, got)


def test_the_wide_edge_lies_inside_the_rising_cell_s():
    """P - 4 rows inside (|ge| > 0): the batches of tests/test_sw_range_*.py, which stand on the rising cell's last ll, stay
    narrow whatever they launch."""
    seen = 0
    for scoring, (ll_at, _) in ref.CASES.items():
        for ls in ll_at:
            L = ref.last_rising_ll(scoring, ls)
            if L is None or ref.variant(scoring, ls, L) != ("biased", 4):
                continue
            for P in sorted({pref.period(c) for c in pref.PACKED_CLASSES} - {pref.NARROW}):
                assert not pref.wide(scoring, ls, L, P)
                Lw = pref.last_wide_ll(scoring, ls, P)
                assert Lw is None or Lw == L - (P - 4), (scoring, ls, P, L, Lw)
                seen += 1
    assert seen
    got = _trace(REF, _pairs([(150, 30490), (150, 30491)]), AGX_SW_FORCE_C="38")
    assert got == [(4, 4, 19), (0, None, None)], got


def test_headline_configs_plan_wide():
    """BASELINE config 2 (65 536 pairs of 150 x 150) as 4 lanes of 38 columns at period 19, and mixed lengths 32 .. 512 (config 4) at
    the period of the widest class they launch."""
    assert pref.wide(REF, 151, 151, 20) and pref.wide(REF, 513, 513, 20)
    got = _trace(REF, [["synth", 65536, 150, 150, 2], ["synth", 65536, 32, 512, 4]])
    assert got[0] == (4, pref.period(38), pref.period(38)), got
    assert got[1][0] == 4 and got[1][1] == got[1][2] and got[1][1] > pref.NARROW, got


def test_knob_forces_the_narrow_period():
    got = _trace(REF, [["synth", 65536, 150, 150, 2]], AGX_SW_PERIOD="4")
    assert got == [(4, pref.NARROW, pref.period(38))], got


def test_other_cells_have_no_class_period():
    """KC = 1 and the plain cell print no such line; lanes narrower than 14 columns have no column classes to widen."""
    assert _trace((1, -2, -3, -1), _pairs([(150, 150)]), AGX_SW_FORCE_C="38") == [(1, None, None)]
    assert _trace(REF, _pairs([(8, 8)]), AGX_SW_FORCE_C="8") == [(4, 4, 4)]
