"""preAlps_hip_set_band_precision without a GPU: 64, 32 and 0 (follow PREALPS_BJ_BAND_PRECISION) are taken, any other
value is refused with a message in return-code mode; the Python keyword refuses unknown values before it calls the
library."""
import pytest

import prealps_amd as pa


@pytest.mark.parametrize("bits", [0, 32, 64])
def test_set_band_precision_takes_64_32_and_0(bits):
    L = pa.load()
    try:
        assert L.preAlps_hip_set_band_precision(bits) == 0
    finally:
        L.preAlps_hip_set_band_precision(0)


@pytest.mark.parametrize("bits", [16, -1])
def test_set_band_precision_refuses_other_values(bits):
    L = pa.load()
    try:
        assert L.preAlps_hip_set_band_precision(bits) != 0
        msg = L.preAlps_hip_last_error().decode()
        assert "preAlps_hip_set_band_precision" in msg and ("precision %d refused" % bits) in msg
    finally:
        L.preAlps_hip_set_band_precision(0)


def test_the_two_precision_entries_do_not_share_their_setting():
    """A refused value of one entry leaves the other's accepted value alone (both are plain settings, no GPU)."""
    L = pa.load()
    try:
        assert L.preAlps_hip_set_nd_precision(32) == 0
        assert L.preAlps_hip_set_band_precision(16) != 0
        assert L.preAlps_hip_set_band_precision(64) == 0
        assert L.preAlps_hip_set_nd_precision(0) == 0
    finally:
        L.preAlps_hip_set_nd_precision(0)
        L.preAlps_hip_set_band_precision(0)


def test_python_keyword_refuses_unknown_values():
    """create_block_jacobi(band_precision="half") raises ValueError before anything reaches the library (no GPU, no
    operator: the check comes first)."""
    from prealps_amd.solver import EcgProblem
    prob = EcgProblem.__new__(EcgProblem)          # (no device: only the argument check runs)
    with pytest.raises(ValueError, match="band_precision"):
        prob.create_block_jacobi(band_precision="half")
