"""The moment passes keep their bits: every output of points_alignment (forward and backward), of three IcpState steps
and of three RegistrationState steps of either estimation, at the shapes of tests/moment_passes_cases.py, compared with
NO tolerance against tests/golden/moment_passes.npz: per case the bytes these calls write on an MI355X, outputs only
(the inputs come from synth seeds).

The float64 bounds of the alignment and registration tests would let a changed summation order pass; this does not.
Most statements of pa_accumulate feed accumulators of their own, so swapping them changes no bit; what the bytes pin is
the order WITHIN a sum: the a-ascending |x|^2 of pa_accumulate, the walk of the rows, block_sum.h's wave and block
reduction and the ascending sum of the block partials.

Regenerate the recording with `python tools/record_moment_passes.py` on the GPU -- but only for a DELIBERATE change of
one of those orders.  A refactor that changes these bytes is wrong.  A case without its entry fails; nothing here
skips."""
import pytest

import moment_passes_cases as cases
from conftest import load_golden

pytestmark = pytest.mark.gpu

_GOLDEN = []


def _golden():
    if not _GOLDEN:
        _GOLDEN.append(load_golden("moment_passes"))
    return _GOLDEN[0]


@pytest.mark.parametrize("name", cases.case_names())
def test_outputs_are_the_recorded_bytes(dev, name):
    golden = _golden()
    assert name in golden.files, f"tests/golden/moment_passes.npz has no entry for {name}"
    want = golden[name].tobytes()
    at = 0
    for field, got in cases.compute(name, dev):
        assert got == want[at:at + len(got)], f"{name}: {field} differs from the recording"
        at += len(got)
    assert at == len(want), f"{name}: the recording holds {len(want)} bytes, the outputs {at}"


def test_recording_holds_exactly_the_cases():
    assert sorted(_golden().files) == sorted(cases.case_names())
