"""MS-SSIM targets on the host (codec.py): the value check, the fifth rate option,
the search with fake probes under the MS-SSIM pass rule, the size rule and the command line.
No GPU."""
import math

import numpy as np
import pytest

from iclr_17_compression_amd import codec, kernels
from iclr_17_compression_amd._lib import Iclr17Error
from iclr_17_compression_amd.model import ImageCompressor

STEPS = codec.STEPS
NAN = float("nan")


# ------------------------------------------------------------------------------ the value
def test_msssim_value():
    for good in (0.97, np.float32(0.5), np.float64(0.999), 1e-9, 1.0 - 1e-9):
        assert codec.msssim_value(good) == float(good)
    for bad in (True, False, "0.9", None, [0.9]):
        with pytest.raises(Iclr17Error, match="msssim must be a real number"):
            codec.msssim_value(bad)
    for bad in (0, 0.0, 1, 1.0, -0.5, 1.5, NAN, float("inf"), -float("inf")):
        with pytest.raises(Iclr17Error, match="msssim must be finite, > 0 and < 1"):
            codec.msssim_value(bad)


# ------------------------------------------------------------------------------ rate_request
def test_rate_request_msssim():
    assert codec.rate_request(3, msssim=0.97) == ("msssim", [0.97, 0.97, 0.97])
    assert codec.rate_request(3, msssim=[0.9, 0.95, np.float64(0.99)]) == ("msssim", [0.9, 0.95, 0.99])
    assert codec.rate_request(2, msssim=np.array([0.9, 0.5]), tile=16) == ("msssim", [0.9, 0.5])
    assert codec.rate_request(1, msssim=np.float32(0.5), estimate=False) == ("msssim", [0.5])
    with pytest.raises(Iclr17Error, match="msssim has 2 values for 3 images"):
        codec.rate_request(3, msssim=[0.9, 0.95])
    for kw, names in (({"step": 8}, "step and msssim"), ({"max_bytes": 1000}, "max_bytes and msssim"),
                      ({"bpp": 1.0}, "bpp and msssim"), ({"psnr": 30.0}, "psnr and msssim"),
                      ({"step": 8, "bpp": 1.0}, "step and bpp and msssim"),
                      ({"bpp": 1.0, "psnr": 30.0}, "bpp and psnr and msssim")):
        with pytest.raises(Iclr17Error) as e:
            codec.rate_request(3, msssim=0.9, **kw)
        options = "step, max_bytes, bpp, psnr, msssim" if "psnr" in kw else "step, max_bytes, bpp, msssim"
        assert f"{names} given together (at most one of {options})" in str(e.value)
    with pytest.raises(Iclr17Error, match="msssim with rdo.*is not built"):
        codec.rate_request(3, msssim=0.9, rdo=1.0)
    with pytest.raises(Iclr17Error, match="msssim with step_offsets.*is not built"):
        codec.rate_request(3, msssim=0.9, step_offsets=[None] * 3)
    with pytest.raises(Iclr17Error, match="msssim with estimate=True.*is not built"):
        codec.rate_request(3, msssim=0.9, estimate=True)
    with pytest.raises(Iclr17Error, match="tiled step maps are not built"):
        codec.rate_request(3, msssim=0.9, step_offsets=[None] * 3, tile=8)
    with pytest.raises(Iclr17Error, match="tile must be one of"):
        codec.rate_request(3, msssim=0.9, tile=7)
    for bad in (True, "0.9", NAN, float("inf"), 0.0, 1.0, -1, [0.9, True, 0.8], [0.9, NAN, 0.8]):
        with pytest.raises(Iclr17Error, match="msssim must be"):
            codec.rate_request(3, msssim=bad)


# literal expectations, copied from the behaviour before msssim existed
UNCHANGED = [
    ({}, None),
    ({"tile": 16}, None),
    ({"step": 0}, ("step", 0)),
    ({"step": 31, "tile": 8}, ("step", 31)),
    ({"rdo": 0.5}, ("step", 8)),
    ({"rdo": 0.5, "step": 3}, ("step", 3)),
    ({"step_offsets": [None] * 3}, ("step", 8)),
    ({"step_offsets": [None] * 3, "step": 12}, ("step", 12)),
    ({"max_bytes": 900}, ("budget", [900.0, 900.0, 900.0], False)),
    ({"max_bytes": [900, 800, 700]}, ("budget", [900.0, 800.0, 700.0], False)),
    ({"bpp": 0.75, "tile": 32}, ("budget", [0.75, 0.75, 0.75], True)),
    ({"bpp": np.array([0.5, 1.0, 2.0]), "rdo": 2.0}, ("budget", [0.5, 1.0, 2.0], True)),
    ({"step_offsets": [None] * 3, "max_bytes": 500}, ("budget", [500.0, 500.0, 500.0], False)),
    ({"psnr": 32}, ("quality", [32.0, 32.0, 32.0])),
    ({"psnr": [30, 31.5, np.float64(40)], "tile": 8}, ("quality", [30.0, 31.5, 40.0])),
]
UNCHANGED_ERRORS = [
    ({"step": 8, "max_bytes": 1000},
     "iclr17: codec: step and max_bytes given together (at most one of step, max_bytes, bpp)"),
    ({"max_bytes": 1000, "bpp": 1.0},
     "iclr17: codec: max_bytes and bpp given together (at most one of step, max_bytes, bpp)"),
    ({"step": 8, "psnr": 30.0},
     "iclr17: codec: step and psnr given together (at most one of step, max_bytes, bpp, psnr)"),
    ({"step": 8, "bpp": 1.0, "psnr": 30.0},
     "iclr17: codec: step and bpp and psnr given together (at most one of step, max_bytes, bpp, psnr)"),
    ({"tile": 8, "step_offsets": [None] * 3},
     "iclr17: codec: tile with step_offsets / a step map: tiled step maps are not built"),
    ({"rdo": 1.0, "step_offsets": [None] * 3},
     "iclr17: codec: rdo with step_offsets / a step map: per-block rate–distortion optimised "
     "quantisation is not built"),
    ({"psnr": 30.0, "rdo": 1.0},
     "iclr17: codec: psnr with rdo: a quality target over rate–distortion optimised levels is not built"),
    ({"psnr": 30.0, "step_offsets": [None] * 3},
     "iclr17: codec: psnr with step_offsets / a step map: a quality target over per-block steps is "
     "not built"),
    ({"psnr": [30.0, 31.0]}, "iclr17: codec: psnr has 2 values for 3 images"),
    ({"psnr": -1}, "iclr17: codec: psnr must be finite and > 0 (got -1)"),
    ({"bpp": -1.0}, "iclr17: codec: bpp must be finite and positive"),
    ({"max_bytes": [1, 2]}, "iclr17: codec: max_bytes has 2 values for 3 images"),
    ({"step": 32}, "iclr17: codec: quantiser step index 32 is not an integer in 0..31"),
    ({"tile": 7}, "iclr17: codec: tile must be one of (8, 16, 32, 64) latent positions (got 7)"),
    ({"rdo": -0.5}, "iclr17: codec: rdo must be finite and >= 0 (got -0.5)"),
]


def test_rate_request_without_msssim_is_unchanged():
    def plain(r):
        if r is None or r[0] == "step":
            return r
        return (r[0], [float(v) for v in r[1]]) + tuple(r[2:])

    for kw, want in UNCHANGED:
        for extra in ({}, {"msssim": None}, {"msssim": None, "estimate": True}):
            if "psnr" in kw and extra.get("estimate"):
                continue
            assert plain(codec.rate_request(3, **kw, **extra)) == want, kw
    for kw, text in UNCHANGED_ERRORS:
        for extra in ({}, {"msssim": None}):
            with pytest.raises(Iclr17Error) as e:
                codec.rate_request(3, **kw, **extra)
            assert str(e.value) == text, kw


# ------------------------------------------------------------------------------ the search
def targets(values):
    return [codec.MsssimTarget(f"image {k} (200x300)", T, 200, 300) for k, T in enumerate(values)]


class Probe:
    """A fake probe over per-image rows of 32 MS-SSIM values; it records every call and asserts
    the search's own rules: members ascending and unfinished, an index strictly inside the bracket
    that the earlier answers gave."""

    def __init__(self, tables, wanted):
        self.tables, self.wanted = tables, wanted
        n = len(tables)
        self.lo, self.hi = [-1] * n, [STEPS] * n
        self.history = [[] for _ in range(n)]

    def __call__(self, members, indices):
        assert members == sorted(set(members)) and len(members) == len(indices)
        out = []
        for k, s in zip(members, indices):
            assert self.hi[k] > self.lo[k] + 1, "a finished image was probed again"
            assert isinstance(s, int) and self.lo[k] < s < self.hi[k]
            self.history[k].append(s)
            v = self.tables[k][s]
            if v >= self.wanted[k]:
                self.lo[k] = s
            else:
                self.hi[k] = s
            out.append(v)
        return out


def search(tables, wanted):
    probe = Probe(tables, wanted)
    found = codec.search_quality(probe, len(tables), None, targets(wanted), codec.msssim_passes,
                                 codec.msssim_failure)
    return found, probe


def check(found, probe, tables, wanted):
    for k, (row, T) in enumerate(zip(tables, wanted)):
        L = found.indices[k]
        assert row[L] >= T and (L == STEPS - 1 or not row[L + 1] >= T), (k, L)
        assert L in probe.history[k] and (L == STEPS - 1 or L + 1 in probe.history[k])
        assert found.probes[k] == len(probe.history[k]) <= 6
        assert found.sse[k] == row[L] and isinstance(found.sse[k], float)
    assert found.guesses == [None] * len(tables)


def falling(boundary):
    """MS-SSIM falling along the ladder: ≥ 0.9 below ``boundary``, < 0.9 from it on."""
    return [0.9 + 0.001 * (boundary - s) if s < boundary else 0.9 - 0.002 * (s - boundary + 1)
            for s in range(STEPS)]


def test_monotone_rows_find_the_boundary():
    tables = [falling(b) for b in range(1, STEPS + 1)]
    found, probe = search(tables, [0.9] * len(tables))
    check(found, probe, tables, [0.9] * len(tables))
    assert found.indices == [b - 1 for b in range(1, STEPS + 1)]     # all pass: 31


def test_exact_equality_passes_and_nothing_is_rounded():
    row = [0.97] * 16 + [math.nextafter(0.97, 0.0)] * 16
    found, probe = search([row], [0.97])
    assert found.indices == [15]
    found, _ = search([row], [math.nextafter(0.97, 0.0)])    # one ulp lower: every index passes
    assert found.indices == [STEPS - 1]


def test_non_monotone_rows_keep_the_local_contract():
    rng = np.random.default_rng(7)
    tables, wanted = [], []
    for _ in range(40):
        row = [float(v) for v in rng.uniform(0.5, 0.99, STEPS)]
        row[0] = 0.995                                       # index 0 passes whatever else does
        tables.append(row)
        wanted.append(float(rng.uniform(0.6, 0.95)))
    found, probe = search(tables, wanted)
    check(found, probe, tables, wanted)


def test_nan_counts_as_a_fail():
    row = falling(20)
    for s in (10, 15, 17):
        row[s] = NAN                                         # 15 is the first probe of a bisection
    found, probe = search([row], [0.9])
    check(found, probe, [row], [0.9])
    assert probe.history[0][0] == 15 and found.indices[0] < 15
    with pytest.raises(Iclr17Error, match=r"image 0 \(200x300\) cannot reach MS-SSIM 0.9: .*gives nan"):
        search([[NAN] * STEPS], [0.9])


def test_all_fail_raises_with_the_value_at_index_zero():
    tables = [falling(32), [0.5 + 0.001 * s for s in range(STEPS)], falling(4)]
    with pytest.raises(Iclr17Error) as e:
        search(tables, [0.9, 0.9, 0.9])
    assert str(e.value) == ("iclr17: codec: image 1 (200x300) cannot reach MS-SSIM 0.9: the finest "
                            "step (index 0) gives 0.5")
    T = math.nextafter(0.97, 1.0)                            # one ulp above what index 0 reaches
    with pytest.raises(Iclr17Error, match=rf"cannot reach MS-SSIM {T!r}: .*gives 0.97"):
        search([[0.97] * STEPS], [T])


def test_an_image_alone_probes_as_in_its_batch():
    rng = np.random.default_rng(11)
    tables = [falling(3), falling(32), [0.995] + [float(v) for v in rng.uniform(0.5, 0.99, STEPS - 1)],
              falling(17)]
    wanted = [0.9, 0.9, 0.8, 0.9]
    found, probe = search(tables, wanted)
    check(found, probe, tables, wanted)
    for k in range(len(tables)):
        alone, alone_probe = search([tables[k]], [wanted[k]])
        assert alone_probe.history[0] == probe.history[k]
        assert (alone.indices, alone.probes, alone.sse) == ([found.indices[k]], [found.probes[k]],
                                                            [found.sse[k]])


# ------------------------------------------------------------------------------ the size rule
def test_too_small_images_raise_before_any_device_use():
    kernels.check_msssim_shapes([(161, 161), (161, 4000), (1000, 161)])
    for shape in ((160, 300), (300, 160), (10, 10)):
        with pytest.raises(Iclr17Error, match="too small for 5 levels of an 11-tap window"):
            kernels.check_msssim_shapes([(161, 161), shape])
    # the library's own rule (level_plan): five levels of ⌈n/2⌉, each at least 11
    def levels_fit(n):
        for _ in range(5):
            if n < 11:
                return False
            n = (n + 2 * (n % 2) - 2) // 2 + 1
        return True
    assert [n for n in range(1, 400) if levels_fit(n)][0] == kernels.MSSSIM_MIN_SIDE == 161
    assert all(levels_fit(n) for n in range(161, 400))
    net = ImageCompressor(128).eval()     # on the CPU: whatever reached the device would raise
    ok, small = np.zeros((161, 161, 3), np.uint8), np.zeros((160, 300, 3), np.uint8)
    for call in (net.compress_images, net.evaluate_images):
        with pytest.raises(Iclr17Error, match=r"image 1 \(160x300\) is 160x300, too small"):
            call([ok, small], msssim=0.9)
        with pytest.raises(RuntimeError) as e:               # 161×161 passes the check: the
            call([ok], msssim=0.9)                           # upload is what fails without a GPU
        assert "too small" not in str(e.value) and "GPU" in str(e.value)
        for kw, text in (({"rdo": 1.0}, "msssim with rdo"), ({"estimate": True}, "msssim with estimate"),
                         ({"step": 3}, "step and msssim given together")):
            with pytest.raises(Iclr17Error, match=text):
                call([ok], msssim=0.9, **kw)
        with pytest.raises(Iclr17Error, match="msssim must be"):
            call([ok], msssim=1.0)


# ------------------------------------------------------------------------------ the command line
def test_command_line_parsing():
    p = codec.build_parser()
    a = p.parse_args(["encode", "in.png", "out.i17c", "--weights", "w.pth", "--msssim", "0.97"])
    assert a.msssim == 0.97 and a.step is None and a.psnr is None
    a = p.parse_args(["encode", "i", "o", "--weights", "w", "--msssim", "0.9", "--tile", "16"])
    assert a.msssim == 0.9 and a.tile == 16
    assert p.parse_args(["encode", "i", "o", "--weights", "w"]).msssim is None
    for other in (["--step", "8"], ["--max-bytes", "100"], ["--bpp", "1.0"], ["--psnr", "30"]):
        with pytest.raises(SystemExit):
            p.parse_args(["encode", "i", "o", "--weights", "w", "--msssim", "0.9", *other])
    e = p.parse_args(["eval", "a.png", "b.png", "--weights", "w", "--msssim", "0.95"])
    assert e.msssim == 0.95 and e.psnr is None and e.steps is None
    for argv, text in ((["encode", "i", "o", "--weights", "w", "--msssim", "0.9", "--rdo", "1"],
                        "msssim with rdo"),
                       (["encode", "i", "o", "--weights", "w", "--msssim", "0.9", "--roi", "0,0,8,8,-2"],
                        "msssim with step_offsets"),
                       (["eval", "a.png", "--weights", "w", "--msssim", "0.9", "--steps", "4,8"],
                        "step and msssim given together"),
                       (["eval", "a.png", "--weights", "w", "--msssim", "0.9", "--psnr", "30"],
                        "psnr and msssim given together"),
                       (["encode", "i", "o", "--weights", "w", "--msssim", "1.5"], "msssim must be")):
        with pytest.raises(Iclr17Error) as err:
            codec.main(argv)
        assert text in str(err.value)
