"""The depthwise convolution width rule (odd, 1 to 63), without a GPU: the check the modules and the binding share."""
import pytest

from fastspeech2_lightning_amd import hip as H


@pytest.mark.parametrize("k", [1, 3, 9, 11, 17, 31, 33, 63])
def test_odd_widths_up_to_63_are_taken(k):
    assert H.dwconv_width_ok(k)


@pytest.mark.parametrize("k", [0, -1, 2, 8, 64, 65, 127])
def test_other_widths_are_refused(k):
    assert not H.dwconv_width_ok(k)
    assert "odd, 1 to 63" in H.DWCONV_WIDTHS
