"""The --master option of the headless driver (termdaw_amd/__main__.py), on the host: LUFS alone or LUFS:DBTP, in the
space-separated form the README shows as well as the `=` form, and malformed values refused."""
import pytest

from termdaw_amd import __main__ as M
from termdaw_amd import api


@pytest.mark.parametrize("argv,want", [(["--master", "-14:-1"], ["--master=-14:-1"]),
                                       (["d", "--master", "-16", "-o", "x.wav"], ["d", "--master=-16", "-o", "x.wav"]),
                                       (["d", "--master=-23:-2"], ["d", "--master=-23:-2"]),
                                       (["d", "--master"], ["d", "--master"])])
def test_master_value_is_joined(argv, want):
    assert M.join_master_value(argv) == want


@pytest.mark.parametrize("text,want", [("-14", (-14.0, -1.0)), ("-14:-1", (-14.0, -1.0)), ("-23:-2.5", (-23.0, -2.5)), ("0:0", (0.0, 0.0))])
def test_parse_master(text, want):
    assert M.parse_master(text) == want


@pytest.mark.parametrize("text", ["", "loud", "-14:", "-14:-1:-2", ":-1"])
def test_parse_master_refuses_malformed_values(text):
    with pytest.raises(api.TermdawError, match="--master"):
        M.parse_master(text)
