"""GPU: the five colour difference entries of the deltae command (csrc/delta_e.hip, receptor.hip, scielab.hip, receptor_acuity.hip,
itp.hip) write, bit for bit, what they wrote when tests/golden/deltae_family_digests.json was recorded: the float32 values, the maps and
the raw records of the cases of tests/_deltae_digests.py.  The value tests of the five entries carry tolerances (1e-3, 2e-4); this one
has none, so a change of a rounding in the code the entries share cannot pass."""
import json
import os

import pytest

import _deltae_digests as D

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deltae_family_digests.json")


def test_every_case_has_the_recorded_digest():
    with open(FIXTURE) as f:
        fixture = json.load(f)
    want, got = fixture["digests"], D.compute()
    assert sorted(got) == sorted(want)
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, (f"{len(differ)} of {len(want)} cases differ from the digests recorded from {fixture['recorded_from']} with ROCm {fixture['rocm']}: "
                        f"{', '.join(differ)}.  A digest that differs is a changed bit in a value, a map or a record: explain it from the code.  The fixture "
                        "is re-recorded (python tests/_deltae_digests.py) only from a commit whose deltae tests pass, and only when the toolchain changed.")
