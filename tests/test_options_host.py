"""The run-time options (include/fmrx.h, csrc/options.cpp) without a GPU: fmrx_set_option / fmrx_get_option never touch HIP.
What is checked here is written from the header's description, not read from the library: defaults, ranges, named values, and
the one-time read of the environment (in a fresh child process per case, since the library reads it once)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
LONG_MIN, LONG_MAX = -2 ** 63, 2 ** 63 - 1

# name -> (default, lowest, highest)
OPTIONS = {
    "fe_variant": (0, 0, 1),
    "fused_min_audio": (65536, LONG_MIN, LONG_MAX),
    "resample_l2": (0, INT_MIN, INT_MAX),
    "resample_exact": (0, INT_MIN, INT_MAX),
    "resample_chains": (0, INT_MIN, INT_MAX),
    "overlap_calls": (0, INT_MIN, INT_MAX),
    "pll_warmup": (-1, INT_MIN, INT_MAX),
    "pll_segment": (-1, INT_MIN, INT_MAX),
    "pll_start": (1, INT_MIN, INT_MAX),
    "pll_mode": (0, 0, 2),
    "demod": (0, 0, 1),
    "tuner_variant": (0, 0, 1),
    "deemph_warmup": (-1, -1, 2 ** 20),
    "deemph_segment": (-1, -1, 2 ** 20),
    "deemph_mode": (0, 0, 1),
}
NAMED = {"fe_variant": {"mfma": 0, "valu": 1}, "tuner_variant": {"mfma": 0, "generic": 1},
         "demod": {"discriminator": 0, "arctan": 1}}

CHILD = ("import importlib, json, sys; m = importlib.import_module('software-defined-radio_amd'); "
         "print(json.dumps({n: m.get_option(n) for n in sys.argv[1:]}))")


def child_options(env_vars):
    """every option as a fresh process sees it with only these FMRX_* variables set -> (values, stderr)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("FMRX_") or k == "FMRX_LIB"}
    env.update(env_vars)
    r = subprocess.run([sys.executable, "-c", CHILD, *OPTIONS], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout), r.stderr


@pytest.fixture
def restored(fmrx):
    before = {n: fmrx.get_option(n) for n in OPTIONS}
    yield fmrx
    for n, v in before.items():
        fmrx.set_option(n, v)


def test_defaults_are_the_documented_ones():
    got, err = child_options({})
    assert got == {n: d for n, (d, _, _) in OPTIONS.items()}
    assert err == ""


@pytest.mark.parametrize("name", OPTIONS)
def test_round_trip_and_range(restored, name):
    fmrx = restored
    _, lo, hi = OPTIONS[name]
    for v in (lo, hi):
        fmrx.set_option(name, v)
        assert fmrx.get_option(name) == v
    if name == "fused_min_audio":
        fmrx.set_option(name, 10 ** 12)
        assert fmrx.get_option(name) == 10 ** 12
        return
    outside = [lo - 1, hi + 1] + ([0] if name == "deemph_segment" else [])
    for v in outside:
        with pytest.raises(fmrx.FmrxError) as e:
            fmrx.set_option(name, v)
        assert e.value.code == fmrx.EINVAL and name in str(e.value)
        assert fmrx.get_option(name) == hi


def test_unknown_name(fmrx):
    for call in (lambda: fmrx.set_option("no_such_option", 0), lambda: fmrx.get_option("no_such_option"),
                 lambda: fmrx.set_option("", 0), lambda: fmrx.set_option("FE_VARIANT", 0)):
        with pytest.raises(fmrx.FmrxError) as e:
            call()
        assert e.value.code == fmrx.EINVAL


def test_named_values_belong_to_their_option(restored):
    fmrx = restored
    for name, values in NAMED.items():
        for word, number in values.items():
            fmrx.set_option(name, word)
            assert fmrx.get_option(name) == number
            for other in OPTIONS:
                if word in NAMED.get(other, {}):
                    continue
                before = fmrx.get_option(other)
                with pytest.raises(fmrx.FmrxError) as e:
                    fmrx.set_option(other, word)
                assert e.value.code == fmrx.EINVAL and fmrx.get_option(other) == before


@pytest.mark.parametrize("pick", [0, 1])
def test_environment_names(pick):
    """FMRX_<NAME>=<name> gives the number Python's set_option gives for that name: the two maps cannot drift"""
    words = {name: list(values)[pick] for name, values in NAMED.items()}
    got, err = child_options({"FMRX_" + name.upper(): w for name, w in words.items()})
    for name, w in words.items():
        assert got[name] == NAMED[name][w], name
    assert err == ""


def test_environment_integers():
    want = {"fe_variant": 1, "fused_min_audio": 10 ** 12, "resample_l2": 3, "resample_exact": 1, "resample_chains": 7,
            "overlap_calls": 2, "pll_warmup": 96, "pll_segment": 128, "pll_start": 0, "pll_mode": 2, "demod": 1,
            "tuner_variant": 1, "deemph_warmup": 0, "deemph_segment": 2 ** 20, "deemph_mode": 1}
    assert set(want) == set(OPTIONS) and all(want[n] != OPTIONS[n][0] for n in want)
    got, err = child_options({"FMRX_" + n.upper(): str(v) for n, v in want.items()})
    assert got == want and err == ""
    got, err = child_options({"FMRX_RESAMPLE_L2": "0", "FMRX_PLL_WARMUP": "-5"})
    assert got["resample_l2"] == 0 and got["pll_warmup"] == -5 and err == ""


@pytest.mark.parametrize("var,value", [("FMRX_DEEMPH_SEGMENT", "0"), ("FMRX_PLL_MODE", "7"), ("FMRX_DEMOD", "1x"),
                                       ("FMRX_FE_VARIANT", "generic"), ("FMRX_PLL_SEGMENT", str(2 ** 31)), ("FMRX_PLL_START", "")])
def test_environment_rejects(var, value):
    got, err = child_options({var: value})
    assert got == {n: d for n, (d, _, _) in OPTIONS.items()}
    lines = err.strip().splitlines()
    assert len(lines) == 1 and var in lines[0] and (value in lines[0])
