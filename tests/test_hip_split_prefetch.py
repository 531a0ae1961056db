"""Split-K with two or more stages per split on a bf16 tile whose last column group is partly idle (Np no multiple of
32 * NB: 136 channels on the four-block tile): the waves without live columns still stage their share of every box and
must prefetch the next stage like the others.  At the launch geometry of 24 volumes in flight (split-K below 16
workgroups, target 22) the 128 -> 136 layer of tests/test_hip_conv.py runs 4 splits of 2 stages; before the fix the
idle waves committed the previous stage's registers."""
import pytest

from test_hip_conv import test_conv_bf16_operands, test_conv_bf16_stored_activations

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _default_launch_geometry():
    """The launch-geometry knobs (options 2 - 5 and 12) are process wide and a plugin test that ran earlier may have tuned
    them: this module runs at the library defaults (4 volumes in flight) and leaves the knobs as it found them."""
    import conv_geometry
    with conv_geometry.pinned(conv_geometry.inflight_values(4)):
        yield

CASE = (128, 136, 3, 1, False, (2, 4, 6, 8))


@pytest.mark.parametrize("below,target", [(16, 22), (96, 256)])
@pytest.mark.parametrize("check", [test_conv_bf16_operands, test_conv_bf16_stored_activations])
def test_split_stages_with_idle_column_waves(check, below, target):
    from multimodal_tta_amd import ops
    prev = (ops.set_option(2, below), ops.set_option(3, target))
    try:
        check(*CASE)
    finally:
        ops.set_option(2, prev[0])
        ops.set_option(3, prev[1])
