"""preAlps_hip_set_nd_precision without a GPU: 64, 32 and 0 (follow PREALPS_BJ_ND_PRECISION) are taken, any other
value is refused with a message in return-code mode."""
import pytest

import prealps_amd as pa


@pytest.mark.parametrize("bits", [0, 32, 64])
def test_set_nd_precision_takes_64_32_and_0(bits):
    L = pa.load()
    try:
        assert L.preAlps_hip_set_nd_precision(bits) == 0
    finally:
        L.preAlps_hip_set_nd_precision(0)


@pytest.mark.parametrize("bits", [16, -1])
def test_set_nd_precision_refuses_other_values(bits):
    L = pa.load()
    try:
        assert L.preAlps_hip_set_nd_precision(bits) != 0
        msg = L.preAlps_hip_last_error().decode()
        assert "preAlps_hip_set_nd_precision" in msg and ("precision %d refused" % bits) in msg
    finally:
        L.preAlps_hip_set_nd_precision(0)
