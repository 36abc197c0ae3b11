"""Quality targets on the host (codec.py): the search with fake probes, the SSE
limit, the new rate option and the command line. No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

from iclr_17_compression_amd import codec
from iclr_17_compression_amd._lib import Iclr17Error

STEPS = codec.STEPS


def targets(n, limit=1000):
    return [codec.QualityTarget(f"image {k} (8x8)", 30.0, 8, 8, limit) for k in range(n)]


class Probe:
    """A fake probe over per-image tables of 32 SSEs; it records every call and asserts the
    search's own rules: one call per round, members ascending and unfinished, an index strictly
    inside the bracket that the earlier answers gave."""

    def __init__(self, tables, limits):
        self.tables, self.limits = tables, limits
        n = len(tables)
        self.lo, self.hi = [-1] * n, [STEPS] * n
        self.history = [[] for _ in range(n)]
        self.rounds = []

    def __call__(self, members, indices):
        assert members == sorted(set(members)) and len(members) == len(indices)
        self.rounds.append(list(members))
        out = []
        for k, s in zip(members, indices):
            assert self.hi[k] > self.lo[k] + 1, "a finished image was probed again"
            assert isinstance(s, int) and self.lo[k] < s < self.hi[k], (k, s, self.lo[k], self.hi[k])
            self.history[k].append(s)
            e = int(self.tables[k][s])
            if e <= self.limits[k]:
                self.lo[k] = s
            else:
                self.hi[k] = s
            out.append(e)
        return out


def monotone_table(boundary, limit=1000):
    """SSEs that pass (≤ limit) below ``boundary`` and fail from it on, rising along the ladder."""
    return [limit - (boundary - s) * 3 if s < boundary else limit + 1 + (s - boundary) * 5
            for s in range(STEPS)]


def seed_for(table, rng, kind):
    """A guided search's seed for a table: exact, noisy, misleading or absent."""
    t = np.asarray(table, dtype=np.float64)
    if kind == "none":
        return None
    if kind == "exact":
        return t - t.min() + 1.0
    if kind == "noisy":
        return np.maximum(t * rng.uniform(0.3, 3.0, STEPS), 0.0)
    if kind == "reverse":
        return t[::-1].copy()
    return rng.uniform(0.0, 5000.0, STEPS)          # "random"


SEED_KINDS = ("none", "exact", "noisy", "reverse", "random")


def check_contract(found, probe, tables, limits):
    for k, table in enumerate(tables):
        L = found.indices[k]
        assert 0 <= L < STEPS and table[L] <= limits[k]                 # the answer passed
        assert L in probe.history[k]                                     # and was measured
        assert found.sse[k] == table[L]
        if L < STEPS - 1:                                                # its neighbour failed,
            assert L + 1 in probe.history[k] and table[L + 1] > limits[k]   # measured
        assert found.probes[k] == len(probe.history[k]) <= codec.MAX_PROBES
        assert len(set(probe.history[k])) == len(probe.history[k])


def test_monotone_boundaries_every_seed_kind():
    rng = np.random.default_rng(17)
    for boundary in range(1, STEPS + 1):          # 0 is the unreachable case below
        table = monotone_table(boundary)
        for kind in SEED_KINDS:
            for _ in range(1 if kind in ("none", "exact", "reverse") else 4):
                seed = seed_for(table, rng, kind)
                probe = Probe([table], [1000])
                found = codec.search_quality(probe, 1, None if seed is None else [seed], targets(1))
                assert found.indices == [boundary - 1], (boundary, kind)
                check_contract(found, probe, [table], [1000])
                if kind == "none":
                    assert found.probes[0] <= 6 and found.guesses == [None]
                else:
                    assert probe.history[0][0] == codec.UNIT_STEP


def test_boundary_zero_is_unreachable():
    table = monotone_table(0)
    for seeds in (None, [np.asarray(table, dtype=np.float64)]):
        probe = Probe([table], [1000])
        t = [codec.QualityTarget("image 3 (8x8)", 41.5, 8, 8, 1000)]
        with pytest.raises(Iclr17Error, match=r"image 3 \(8x8\) cannot reach 41\.5 dB") as e:
            codec.search_quality(probe, 1, seeds, t)
        reached = 10.0 * math.log10(255.0 ** 2 * 3 * 64 / table[0])
        assert f"{reached:.4f} dB" in str(e.value) and "index 0" in str(e.value)
        assert 0 in probe.history[0] and len(probe.history[0]) <= codec.MAX_PROBES


def test_non_monotone_tables_keep_the_local_contract():
    rng = np.random.default_rng(2017)
    for case in range(200):
        passes = rng.random(STEPS) < rng.uniform(0.2, 0.8)
        passes[0] = True                              # reachable: the search ends on an index
        table = [int(rng.integers(0, 1001)) if p else int(rng.integers(1001, 5000)) for p in passes]
        kind = SEED_KINDS[case % len(SEED_KINDS)]
        seed = seed_for(table, rng, kind)
        probe = Probe([table], [1000])
        # index 0 passes, so whatever the probes find the bracket cannot end on L = −1 unless
        # index 0 itself was measured failing
        found = codec.search_quality(probe, 1, None if seed is None else [seed], targets(1))
        check_contract(found, probe, [table], [1000])


def test_batch_images_finish_in_different_rounds_and_alone_alike():
    rng = np.random.default_rng(5)
    boundaries = [32, 9, 1, 16, 24]
    limits = [1000, 500, 1000, 77, 1000]
    tables = [monotone_table(b, lim) for b, lim in zip(boundaries, limits)]
    seeds = [None, seed_for(tables[1], rng, "exact"), seed_for(tables[2], rng, "noisy"), None,
             seed_for(tables[4], rng, "random")]
    t = [codec.QualityTarget(f"image {k}", 30.0, 8, 8, lim) for k, lim in enumerate(limits)]
    probe = Probe(tables, limits)
    found = codec.search_quality(probe, 5, seeds, t)
    assert found.indices == [b - 1 for b in boundaries]
    check_contract(found, probe, tables, limits)
    assert len(probe.rounds) == max(found.probes)              # one call per round
    assert len(set(found.probes)) > 1                          # they did finish in different rounds
    for r, members in enumerate(probe.rounds):                 # round r: the images still open
        assert members == [k for k in range(5) if found.probes[k] > r]
    for k in range(5):                                         # alone: the same sequence
        alone = Probe([tables[k]], [limits[k]])
        one = codec.search_quality(alone, 1, [seeds[k]], [t[k]])
        assert alone.history[0] == probe.history[k]
        assert (one.indices[0], one.probes[0], one.sse[0]) == (found.indices[k], found.probes[k],
                                                               found.sse[k])


def test_search_arguments():
    with pytest.raises(Iclr17Error, match="one target"):
        codec.search_quality(lambda m, i: [], 2, None, targets(1))
    with pytest.raises(Iclr17Error, match="one target"):
        codec.search_quality(lambda m, i: [], 1, [None, None], targets(1))
    with pytest.raises(Iclr17Error, match="returned 0 sums"):
        codec.search_quality(lambda m, i: [], 1, None, targets(1))
    assert codec.search_quality(lambda m, i: [], 0, None, []).indices == []


def test_sse_limit():
    assert isinstance(codec.sse_limit(64, 96, 30.0), int)
    for H, W in ((1, 1), (49, 83), (512, 768)):
        peak = 255 ** 2 * 3 * H * W
        last = None
        for T in np.arange(0.5, 80.0, 0.37):
            lim = codec.sse_limit(H, W, float(T))
            assert lim == int(math.floor(255.0 ** 2 * 3.0 * H * W * 10.0 ** (-float(T) / 10.0)))
            assert 0 <= lim <= peak
            assert last is None or lim <= last          # monotone: a higher target, a lower limit
            last = lim
            # an SSE at the limit reaches the target, one above it does not (to float64's rounding
            # of the power: 1e-9 dB)
            if lim:
                assert 10.0 * math.log10(peak / lim) >= float(T) - 1e-9
            assert 10.0 * math.log10(peak / (lim + 1)) <= float(T) + 1e-9
        # exact where 10^(−T/10) is a short decimal: T = 10, 20, 30 dB (the quotient is not an
        # integer multiple away from its floor by less than float64 resolves)
        for T, den in ((10, 10), (20, 100), (30, 1000)):
            exact = Fraction(peak, den)
            if abs(exact - round(exact)) > Fraction(1, 1000):
                assert codec.sse_limit(H, W, T) == exact.numerator // exact.denominator
    for bad in (True, "30", None, float("nan"), float("inf"), 0, -3.0, [30.0]):
        with pytest.raises(Iclr17Error, match="psnr must be"):
            codec.sse_limit(8, 8, bad)
    with pytest.raises(Iclr17Error, match="at least 1x1"):
        codec.sse_limit(0, 8, 30.0)
    assert codec.sse_limit(8, 8, np.float32(30.0)) == codec.sse_limit(8, 8, 30)


# what rate_request answered for every argument set the earlier options allow, recorded before
# psnr existed: (keyword arguments, answer)
EXISTING = [
    ({}, None),
    ({"tile": 16}, None),
    ({"step": 0}, ("step", 0)),
    ({"step": 31, "tile": 8}, ("step", 31)),
    ({"step": np.int64(5)}, ("step", 5)),
    ({"max_bytes": 900}, ("budget", [900, 900, 900], False)),
    ({"max_bytes": [900, 800, 700]}, ("budget", [900, 800, 700], False)),
    ({"bpp": 0.5}, ("budget", [0.5, 0.5, 0.5], True)),
    ({"bpp": [0.5, 1.0, 2.0], "tile": 64}, ("budget", [0.5, 1.0, 2.0], True)),
    ({"rdo": 1.0}, ("step", codec.UNIT_STEP)),
    ({"rdo": 0, "step": 3}, ("step", 3)),
    ({"rdo": 2.0, "bpp": 1.0, "tile": 32}, ("budget", [1.0, 1.0, 1.0], True)),
    ({"step_offsets": [None] * 3}, ("step", codec.UNIT_STEP)),
    ({"step_offsets": [None] * 3, "step": 12}, ("step", 12)),
    ({"step_offsets": [None] * 3, "max_bytes": 500}, ("budget", [500, 500, 500], False)),
]


def test_rate_request_existing_answers_unchanged():
    def plain(r):
        if r is None or r[0] == "step":
            return r
        return r[0], [float(v) for v in r[1]], r[2]

    for kw, want in EXISTING:
        assert plain(codec.rate_request(3, **kw)) == plain(want), kw
        assert plain(codec.rate_request(3, psnr=None, **kw)) == plain(want), kw
    for kw, text in (({"step": 8, "max_bytes": 1000}, "step and max_bytes given together (at most "
                                                      "one of step, max_bytes, bpp)"),
                     ({"tile": 8, "step_offsets": [None] * 3}, "tiled step maps are not built"),
                     ({"rdo": 1.0, "step_offsets": [None] * 3}, "is not built"),
                     ({"bpp": -1.0}, "finite and positive"), ({"step": 32}, "0..31")):
        with pytest.raises(Iclr17Error) as e:
            codec.rate_request(3, **kw)
        assert text in str(e.value)


def test_rate_request_psnr():
    assert codec.rate_request(3, psnr=32) == ("quality", [32.0, 32.0, 32.0])
    assert codec.rate_request(3, psnr=[30, 31.5, np.float64(40)]) == ("quality", [30.0, 31.5, 40.0])
    assert codec.rate_request(2, psnr=np.array([30.0, 33.0]), tile=16) == ("quality", [30.0, 33.0])
    assert codec.rate_request(1, psnr=np.float32(28.5)) == ("quality", [28.5])
    for kw, text in (({"step": 8}, "step and psnr given together"),
                     ({"max_bytes": 1000}, "max_bytes and psnr given together"),
                     ({"bpp": 1.0}, "bpp and psnr given together"),
                     ({"step": 8, "bpp": 1.0}, "step and bpp and psnr given together")):
        with pytest.raises(Iclr17Error) as e:
            codec.rate_request(3, psnr=30.0, **kw)
        assert text in str(e.value) and "at most one of step, max_bytes, bpp, psnr" in str(e.value)
    with pytest.raises(Iclr17Error, match="psnr with rdo.*is not built"):
        codec.rate_request(3, psnr=30.0, rdo=1.0)
    with pytest.raises(Iclr17Error, match="psnr with step_offsets.*is not built"):
        codec.rate_request(3, psnr=30.0, step_offsets=[None] * 3)
    with pytest.raises(Iclr17Error, match="tiled step maps are not built"):
        codec.rate_request(3, psnr=30.0, step_offsets=[None] * 3, tile=8)
    with pytest.raises(Iclr17Error, match="tile must be one of"):
        codec.rate_request(3, psnr=30.0, tile=7)
    with pytest.raises(Iclr17Error, match="psnr has 2 values for 3 images"):
        codec.rate_request(3, psnr=[30.0, 31.0])
    for bad in (True, "30", float("nan"), float("inf"), 0.0, -1, [30.0, True, 31.0],
                [30.0, float("nan"), 31.0]):
        with pytest.raises(Iclr17Error, match="psnr must be"):
            codec.rate_request(3, psnr=bad)


def test_command_line_parsing():
    p = codec.build_parser()
    a = p.parse_args(["encode", "in.png", "out.i17c", "--weights", "w.pth", "--psnr", "32.5"])
    assert a.psnr == 32.5 and a.step is None and a.max_bytes is None and a.bpp is None
    a = p.parse_args(["encode", "in.png", "out.i17c", "--weights", "w.pth", "--psnr", "30",
                      "--tile", "16"])
    assert a.psnr == 30.0 and a.tile == 16
    assert p.parse_args(["encode", "i", "o", "--weights", "w"]).psnr is None
    for other in (["--step", "8"], ["--max-bytes", "100"], ["--bpp", "1.0"]):
        with pytest.raises(SystemExit):
            p.parse_args(["encode", "i", "o", "--weights", "w", "--psnr", "30", *other])
    with pytest.raises(SystemExit):
        p.parse_args(["encode", "i", "o", "--weights", "w", "--psnr", "high"])
    e = p.parse_args(["eval", "a.png", "b.png", "--weights", "w", "--psnr", "34"])
    assert e.psnr == 34.0 and e.images == ["a.png", "b.png"] and e.steps is None
    assert p.parse_args(["eval", "a.png", "--weights", "w"]).psnr is None
    # what cannot go with a target is refused before any device use
    for argv, text in ((["encode", "i", "o", "--weights", "w", "--psnr", "30", "--rdo", "1"],
                        "psnr with rdo"),
                       (["encode", "i", "o", "--weights", "w", "--psnr", "30", "--roi", "0,0,8,8,-2"],
                        "psnr with step_offsets"),
                       (["eval", "a.png", "--weights", "w", "--psnr", "30", "--steps", "4,8"],
                        "step and psnr given together"),
                       (["encode", "i", "o", "--weights", "w", "--psnr", "-3"], "psnr must be")):
        with pytest.raises(Iclr17Error) as err:
            codec.main(argv)
        assert text in str(err.value)
