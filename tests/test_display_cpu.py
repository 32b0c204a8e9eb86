"""Frame statistics, exposure and the display transform without a GPU: the bin rule at its edges, the two host functions
(rm_stats_percentile, rm_stats_exposure: no context, like rm_debug_cull_cell) through ctypes against tests/display_ref.py, every
refusal that needs no context, the ABI, and the hosts' parameter handling."""
import ctypes as C
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import display_ref as DR
from raymarching_engine_amd import abi, capture, dist, job as J, native

ROOT = Path(__file__).resolve().parents[1]
F = np.float32
ENTRY_POINTS = ("rm_frame_stats", "rm_auto_exposure_default", "rm_stats_percentile", "rm_stats_exposure", "rm_display_default", "rm_present_display",
                "rm_present_display_device", "rm_present_linear")
TWO_ULP = 2.4e-7  # two fp32 ulps, relative: the double arithmetic on either side is far tighter, the final rounding may fall either way


def below(x):
    return np.nextafter(F(x), F(-np.inf))


# ---- the bin rule --------------------------------------------------------------------------------------------------------

def test_bin_rule_at_its_edges():
    values = [F(2.0 ** -20), below(2.0 ** -20), F(1.0), below(1.0625), F(1.0625), F(0.18), below(4096.0), F(4096.0)]
    want = [0, -2, 320, 320, 321, 279, 511, -3]
    assert DR.classify(np.array(values, F)).tolist() == want
    odd = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 1e-40, 1e30], F)
    assert DR.classify(odd).tolist() == [-1, -1, -1, -2, -2, -2, -2, -3]
    # the bins tile [2^-20, 2^12): 16 per octave, lo_b the float with the bits (b + 1712) << 19
    e = DR.edge(np.arange(DR.BINS + 1))
    assert e[0] == F(2.0 ** -20) and e[DR.BINS] == F(4096.0) and (np.diff(e.astype(np.float64)) > 0).all()
    assert np.array_equal(e[::16], (2.0 ** np.arange(-20, 13)).astype(F)) and e[321] == F(1.0625)
    assert DR.classify(e[:-1]).tolist() == list(range(DR.BINS))
    assert DR.classify(np.nextafter(e[1:], F(-np.inf))).tolist() == list(range(DR.BINS))


def test_luminance_is_the_firefly_filters():
    import despeckle_ref as D

    rng = np.random.default_rng(2)
    c = (rng.uniform(0.0, 9.0, (7, 9, 4)) * 3).astype(F)
    assert np.array_equal(DR.luminance(c, 3).view(np.uint32), D.luminance(c, 3).view(np.uint32))
    header = (ROOT / "include" / "hip_raymarch.h").read_text()
    assert header.count("(0.2126f * (C.r * s) + 0.7152f * (C.g * s)) + 0.0722f * (C.b * s)") >= 2


# ---- the two host functions ------------------------------------------------------------------------------------------------

def raw_stats(hist, below=0, above=0, non_finite=0):
    s = abi.RmFrameStats(below=below, above=above, non_finite=non_finite)
    hist = np.asarray(hist, np.uint64)
    np.ctypeslib.as_array(s.hist)[:] = hist
    s.pixels = int(hist.sum()) + below + above + non_finite
    return native.FrameStats(s)


def lognormal_luminance(scale=1.0, n=200_000, seed=11):
    rng = np.random.default_rng(seed)
    return (np.exp(rng.normal(np.log(0.3), 1.0, n)) * scale).astype(F)


def _histograms():
    every = np.ones(DR.BINS, np.uint64)
    one_pixel = np.zeros(DR.BINS, np.uint64)
    one_pixel[279] = 1
    one_bin = np.zeros(DR.BINS, np.uint64)
    one_bin[320] = 1000
    return {"empty": np.zeros(DR.BINS, np.uint64), "one pixel": one_pixel, "one bin": one_bin, "every bin once": every,
            "log-normal": DR.stats_of_luminance(lognormal_luminance())["hist"]}


QS = (0.0, 1e-9, 0.001, 0.1, 0.25, 0.5, 0.5000001, 0.75, 0.95, 0.999, 1.0)
EXPOSURES = ({}, dict(key=0.5), dict(low=0.0, high=1.0), dict(low=0.4, high=0.6, key=0.09), dict(low=0.0, high=1e-6), dict(low=0.999, high=1.0),
             dict(min_gain=0.5, max_gain=2.0), dict(min_gain=1.0, max_gain=1.0))


@pytest.mark.parametrize("name", sorted(_histograms()))
def test_host_functions_match_the_restatement(name):
    hist = _histograms()[name]
    st = raw_stats(hist, below=3, above=2, non_finite=1)  # only binned pixels are ranked
    for q in QS:
        got, want = st.percentile(q), DR.percentile(hist, q)
        assert np.float32(got) == want, (q, got, want)
    for fields in EXPOSURES:
        got, want = st.exposure(**fields), float(DR.exposure(hist, **fields))
        assert abs(got - want) <= TWO_ULP * want, (fields, got, want)
    if name == "empty":
        assert st.percentile(0.5) == 0.0 and st.exposure() == 1.0
    if name == "one pixel":
        assert st.percentile(0.0) == st.percentile(1.0) == float(DR.edge(280))
    if name == "every bin once":
        assert st.percentile(0.5) == float(DR.edge(256)) and st.percentile(1.0) == 4096.0


def test_log_average_is_within_half_a_bin_of_the_pixels_own():
    """The histogram's log-average against the float64 log-mean of the same binned pixels: every pixel is within half the width of
    its bin of the bin's geometric centre, and the widest bin (the first of an octave) is log2(17 / 16) wide."""
    bound = np.log2(17.0 / 16.0) / 2.0
    assert abs(bound - 0.0437) < 5e-5
    for scale in (1.0, 1.0 / 64.0, 37.0):
        l = lognormal_luminance(scale)
        cls = DR.classify(l)
        st = DR.stats_of_luminance(l)
        own = float(np.log2(l[cls >= 0].astype(np.float64)).mean())
        m = DR.log_average(st["hist"])
        print(f"scale {scale}: log-average from the histogram {m:.6f}, of the pixels {own:.6f}, difference {m - own:+.6f} octaves (bound {bound:.4f})")
        assert abs(m - own) <= bound
        # and through the library: gain = key / 2^m over the whole histogram
        g = raw_stats(st["hist"]).exposure(low=0.0, high=1.0, key=1.0, min_gain=2.0 ** -30, max_gain=2.0 ** 30)
        assert abs(np.log2(g) + own) <= bound + 1e-6


def test_scaling_by_64_shifts_the_histogram_by_96_bins():
    l = lognormal_luminance()
    a, b = DR.stats_of_luminance(l), DR.stats_of_luminance(l * F(64.0))  # a power of two: exact in fp32
    assert a["below"] == a["above"] == b["below"] == b["above"] == 0  # no pixel near the range ends
    assert np.array_equal(b["hist"][96:], a["hist"][:-96]) and not b["hist"][:96].any() and not a["hist"][-96:].any()
    assert b["min_l"] == a["min_l"] * F(64.0) and b["max_l"] == a["max_l"] * F(64.0)
    sa, sb = raw_stats(a["hist"]), raw_stats(b["hist"])
    for fields in ({}, dict(low=0.0, high=1.0), dict(low=0.3, high=0.7, key=0.4)):
        ga, gb = sa.exposure(**fields), sb.exposure(**fields)
        assert abs(gb - ga / 64.0) <= TWO_ULP * ga / 64.0, (fields, ga, gb)
    for q in QS:
        assert sb.percentile(q) == 64.0 * sa.percentile(q)


def test_every_refusal_of_the_host_functions():
    lib = native.load_library()
    st = raw_stats(_histograms()["log-normal"])
    out = C.c_float(-7.0)
    assert lib.rm_stats_percentile(C.byref(st.raw), 0.5, C.byref(out)) == abi.RM_OK and out.value > 0.0
    assert lib.rm_stats_percentile(None, 0.5, C.byref(out)) == abi.RM_ERR_INVALID
    assert lib.rm_stats_percentile(C.byref(st.raw), 0.5, None) == abi.RM_ERR_INVALID
    for q in (-1e-9, 1.0000001, float("nan"), float("inf"), -float("inf")):
        assert lib.rm_stats_percentile(C.byref(st.raw), q, C.byref(out)) == abi.RM_ERR_INVALID, q
        with pytest.raises(ValueError):
            st.percentile(q)
        with pytest.raises(ValueError):
            DR.percentile(st.hist, q)
    ok = abi.RmAutoExposure()
    lib.rm_auto_exposure_default(C.byref(ok))
    lib.rm_auto_exposure_default(None)  # a NULL block is ignored
    assert lib.rm_stats_exposure(C.byref(st.raw), C.byref(ok), C.byref(out)) == abi.RM_OK
    with_default = out.value
    assert lib.rm_stats_exposure(C.byref(st.raw), None, C.byref(out)) == abi.RM_OK and out.value == with_default  # NULL = the defaults
    assert lib.rm_stats_exposure(None, C.byref(ok), C.byref(out)) == abi.RM_ERR_INVALID
    assert lib.rm_stats_exposure(C.byref(st.raw), C.byref(ok), None) == abi.RM_ERR_INVALID
    nan, inf = float("nan"), float("inf")
    bad = [dict(low=-0.01), dict(low=0.95), dict(low=0.96), dict(high=1.01), dict(high=0.1), dict(low=0.5, high=0.5), dict(key=0.0), dict(key=-1.0),
           dict(min_gain=0.0), dict(min_gain=-1.0), dict(min_gain=2.0, max_gain=1.0), dict(max_gain=2.0 ** -11), dict(reserved=1), dict(reserved=-1)]
    bad += [{name: v} for name in ("key", "low", "high", "min_gain", "max_gain") for v in (nan, inf, -inf)]
    for fields in bad:
        p = abi.RmAutoExposure()
        lib.rm_auto_exposure_default(C.byref(p))
        for name, v in fields.items():
            setattr(p, name, v)
        assert lib.rm_stats_exposure(C.byref(st.raw), C.byref(p), C.byref(out)) == abi.RM_ERR_INVALID, fields
        with pytest.raises(ValueError):
            DR.exposure(st.hist, **fields)
        if "reserved" not in fields:
            with pytest.raises(ValueError):
                st.exposure(**fields)
    # the edges that hold
    for fields in (dict(low=0.0), dict(high=1.0), dict(min_gain=1.0, max_gain=1.0)):
        assert st.exposure(**fields) > 0.0


# ---- ABI ------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_exported_and_declared():
    lib = native.load_library()
    header = (ROOT / "include" / "hip_raymarch.h").read_text()
    for name in ENTRY_POINTS:
        assert name in native.EXPORTS and hasattr(lib, name)
        assert re.search(rf"^RM_API (?:int|void) {name}\(", header, re.M)
    m = re.search(r"#define RM_ABI_VERSION 9 /\* 9: ([^;]*);", header)
    listed = ("RM_STATS_BINS", "RmFrameStats", "RmAutoExposure", "RM_TONE_CLIP", "RmDisplay") + ENTRY_POINTS
    assert m and all(re.search(rf"\b{name}\b", m.group(1)) for name in listed)
    assert lib.rm_abi_version() == 9
    assert re.search(r"RM_TONE_CLIP = 0, RM_TONE_REINHARD = 1, RM_TONE_ACES = 2", header) and re.search(r"#define RM_STATS_BINS 512\b", header)
    assert (abi.RM_TONE_CLIP, abi.RM_TONE_REINHARD, abi.RM_TONE_ACES, abi.RM_STATS_BINS) == (0, 1, 2, 512)
    assert abi.TONE_NAMES == DR.TONES
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
        assert set(ENTRY_POINTS) <= exported


def test_defaults_and_struct_sizes():
    lib = native.load_library()
    d = abi.RmDisplay(gain=9.0, tone=7, white=-1.0, reserved=3)
    lib.rm_display_default(C.byref(d))
    lib.rm_display_default(None)
    assert (d.gain, d.tone, d.white, d.reserved) == (1.0, abi.RM_TONE_CLIP, 4.0, 0)
    assert abi.DISPLAY_DEFAULTS == dict(gain=1.0, tone=0, white=4.0)
    a = abi.RmAutoExposure(reserved=5)
    lib.rm_auto_exposure_default(C.byref(a))
    got = dict(key=a.key, low=a.low, high=a.high, min_gain=a.min_gain, max_gain=a.max_gain)
    assert got == {k: float(F(v)) for k, v in abi.AUTO_EXPOSURE_DEFAULTS.items()} and a.reserved == 0
    assert abi.AUTO_EXPOSURE_DEFAULTS == DR.AUTO_DEFAULTS == dict(key=0.18, low=0.10, high=0.95, min_gain=2.0 ** -10, max_gain=2.0 ** 10)
    assert (C.sizeof(abi.RmFrameStats), C.sizeof(abi.RmAutoExposure), C.sizeof(abi.RmDisplay)) == (4136, 24, 16)
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler to read the struct sizes from the header"
    with tempfile.TemporaryDirectory() as tmp:
        src = Path(tmp) / "s.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hip_raymarch.h"\n'
                       'int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(RmFrameStats), sizeof(RmAutoExposure), sizeof(RmDisplay), '
                       'offsetof(RmFrameStats, non_finite), offsetof(RmFrameStats, min_l), offsetof(RmFrameStats, hist), offsetof(RmAutoExposure, reserved), '
                       'offsetof(RmDisplay, white), RM_STATS_BINS); return 0; }\n')
        subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(Path(tmp) / "s")], check=True)
        out = subprocess.run([str(Path(tmp) / "s")], capture_output=True, text=True, check=True).stdout.split()
        assert [int(x) for x in out] == [4136, 24, 16, abi.RmFrameStats.non_finite.offset, abi.RmFrameStats.min_l.offset, abi.RmFrameStats.hist.offset,
                                         abi.RmAutoExposure.reserved.offset, abi.RmDisplay.white.offset, 512]


DISPLAY_FAULTS = [(dict(gain=0.0), "gain"), (dict(gain=-1.0), "gain"), (dict(gain=float("nan")), "gain"), (dict(gain=float("inf")), "gain"),
                  (dict(tone=-1), "tone"), (dict(tone=3), "tone"), (dict(tone=1, white=0.0), "white"), (dict(tone=1, white=-2.0), "white"),
                  (dict(tone=1, white=float("nan")), "white"), (dict(tone=1, white=float("inf")), "white"), (dict(reserved=1), "reserved")]


def _refusal(lib, which, f, d):
    fp, dp = (C.byref(f) if f is not None else None), (C.byref(d) if d is not None else None)
    if which == "rm_present_display":
        rc = lib.rm_present_display(None, None, 1, fp, dp, None)
    elif which == "rm_present_display_device":
        rc = lib.rm_present_display_device(None, None, 1, fp, dp, None, None)
    else:
        rc = lib.rm_present_linear(None, None, 1, fp, dp, None)
    return rc, lib.rm_last_error(None).decode()


@pytest.mark.parametrize("which", ["rm_present_display", "rm_present_display_device", "rm_present_linear"])
def test_the_display_block_is_checked_first_and_without_a_gpu(which):
    """No context exists without a GPU, so every call ends in RM_ERR_INVALID; the text (rm_last_error(NULL)) tells which check
    spoke: the display block's, then the chain's own values, then the handles."""
    lib = native.load_library()
    rc, msg = _refusal(lib, which, None, None)  # NULL filters = both stages off, NULL display = the default: the handles are NULL
    assert rc == abi.RM_ERR_INVALID and msg == f"{which}: NULL argument"
    for fields, word in DISPLAY_FAULTS:
        d = abi.RmDisplay()
        lib.rm_display_default(C.byref(d))
        for name, v in fields.items():
            setattr(d, name, v)
        bad_chain = native.filters()
        bad_chain.despeckle = 2
        for f in (None, native.filters(despeckle=True), bad_chain):  # the display block speaks before the chain is looked at
            rc, msg = _refusal(lib, which, f, d)
            assert rc == abi.RM_ERR_INVALID and msg.startswith(f"{which}: display") and word in msg, (fields, msg)
    # white is looked at for RM_TONE_REINHARD only
    for tone in (abi.RM_TONE_CLIP, abi.RM_TONE_ACES):
        for white in (0.0, -1.0, float("nan"), float("inf")):
            d = abi.RmDisplay(gain=1.0, tone=tone, white=white)
            rc, msg = _refusal(lib, which, None, d)
            assert rc == abi.RM_ERR_INVALID and msg == f"{which}: NULL argument", (tone, white, msg)
    # after the display block: what rm_present_filtered refuses, in its order
    f = native.filters(despeckle=True)
    f.despeckle_params.rank = 9
    rc, msg = _refusal(lib, which, f, None)
    assert rc == abi.RM_ERR_INVALID and "rank" in msg
    f.despeckle = 0
    rc, msg = _refusal(lib, which, f, None)
    assert rc == abi.RM_ERR_INVALID and msg == f"{which}: NULL argument"


def test_frame_stats_refuses_null_handles_without_a_gpu():
    lib = native.load_library()
    out = abi.RmFrameStats()
    assert lib.rm_frame_stats(None, None, 1, None, C.byref(out)) == abi.RM_ERR_INVALID
    assert lib.rm_last_error(None).decode() == "rm_frame_stats: NULL argument"
    f = native.filters(despeckle=True)
    f.despeckle_params.radius = 5
    assert lib.rm_frame_stats(None, None, 1, C.byref(f), C.byref(out)) == abi.RM_ERR_INVALID
    assert "radius" in lib.rm_last_error(None).decode()


# ---- hosts ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [dict(gain=0.0), dict(gain=-1.0), dict(gain=float("nan")), dict(gain=float("inf")), dict(gain="2"), dict(tone="filmic"),
                                 dict(tone=3), dict(tone=1.5), dict(tone="reinhard", white=0.0), dict(tone=1, white=float("inf")), dict(exposure=1.0),
                                 3, "reinhard", False, abi.RmDisplay(gain=1.0, tone=0, white=4.0, reserved=1)])
def test_python_refuses_bad_display_blocks(bad):
    with pytest.raises(ValueError):
        native.display_params(bad)


def test_python_display_blocks():
    lib = native.load_library()
    d = abi.RmDisplay()
    lib.rm_display_default(C.byref(d))
    assert bytes(native.display_params(None)) == bytes(d) == bytes(native.display_params(True)) == bytes(native.display_params({}))
    p = native.display_params({"gain": 2, "tone": "reinhard", "white": 8.0})
    assert (p.gain, p.tone, p.white, p.reserved) == (2.0, abi.RM_TONE_REINHARD, 8.0, 0)
    assert native.display_params({"tone": "aces", "white": -1.0}).tone == abi.RM_TONE_ACES  # white is the Reinhard operator's alone
    assert native.display_params({"tone": abi.RM_TONE_ACES}).tone == abi.RM_TONE_ACES
    s = abi.RmDisplay(gain=0.5, tone=2, white=1.0)
    assert native.display_params(s) is s
    assert native.display_is_auto("auto") and native.display_is_auto({"auto": True, "tone": "aces"}) and native.display_is_auto({"auto": {"key": 0.3}})
    assert not native.display_is_auto(None) and not native.display_is_auto({"gain": 2.0}) and not native.display_is_auto(s)
    a = native.auto_exposure_params({"key": 0.3})
    assert a.key == float(F(0.3)) and a.low == float(F(0.1))
    for bad in (dict(low=0.9, high=0.2), dict(key=0.0), dict(min_gain=4.0, max_gain=2.0), dict(median=1.0)):
        with pytest.raises(ValueError):
            native.auto_exposure_params(bad)


def test_frame_stats_wrapper_adds_and_views():
    h = _histograms()
    a, b = raw_stats(h["one bin"], below=1, non_finite=2), raw_stats(h["every bin once"], above=4)
    a.raw.min_l, a.raw.max_l, b.raw.min_l, b.raw.max_l = 1.0, 1.03, 2.0 ** -20, 4000.0
    c = a + b
    assert (c.pixels, c.below, c.above, c.non_finite) == (a.pixels + b.pixels, 1, 4, 2) and (c.min, c.max) == (2.0 ** -20, 4000.0)
    assert np.array_equal(c.hist, h["one bin"] + h["every bin once"]) and c.hist.dtype == np.uint64 and c.hist.shape == (512,)
    assert c.pixels == c.below + c.above + c.non_finite + int(c.hist.sum())
    c.hist[0] += 5  # a view of the struct, not a copy
    assert c.raw.hist[0] == 6
    empty = native.FrameStats()
    assert (empty.pixels, empty.min, empty.max) == (0, float("inf"), -float("inf")) and (empty + a).min == 1.0 and (empty + a).pixels == a.pixels


class _Recorder:
    """Stands in for a framebuffer: records how present was called."""
    def __init__(self):
        self.calls = []

    def present(self, samples, **kw):
        self.calls.append((samples, kw))
        return np.zeros((2, 3, 4), np.uint8)


def test_hosts_pass_display_on_and_leave_todays_calls_alone(tmp_path):
    fb = _Recorder()
    capture.save_png(fb, 4, str(tmp_path / "a.png"))
    capture.save_png(fb, 4, str(tmp_path / "b.png"), display="auto")
    capture.save_png(fb, 4, str(tmp_path / "c.png"), denoise=True, despeckle=True, display={"tone": "aces"})
    assert fb.calls == [(4, {}), (4, {"display": "auto"}), (4, {"denoise": True, "despeckle": True, "display": {"tone": "aces"}})]
    fb, frames = _Recorder(), []
    J.collect_presents(frames)(None, None, fb, 2)
    J.collect_presents(frames, display={"auto": True, "tone": "reinhard"})(None, None, fb, 3)
    assert fb.calls == [(2, {}), (3, {"display": {"auto": True, "tone": "reinhard"}})] and len(frames) == 2
    sharded = object.__new__(dist.ShardedFramebuffer)  # nothing set up: a collective would fail on the missing group, not raise ValueError
    with pytest.raises(ValueError, match="sharded"):
        sharded.present(4, display="auto")
