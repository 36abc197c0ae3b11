"""The forward-kernel references and their comparator, checked on the CPU (tests/forward_refs.py):

(a) the GDN / IGDN formula equals oracle.gdn evaluated in float64, and the per-image bit sums add
    up to oracle.estimate_bits: two derivations, equal to 1e-12;
(b) the same formulas evaluated by torch in fp32 pass the comparator at the bars the GPU tests use,
    at every shape those tests run (the bars are 4 × these figures, see forward_refs.BARS), and the
    set of latents a kernel may round the other way stays below 1e-3 of the elements;
(c) planted faults on the float64 reference do not pass at those bars. Each test's docstring says
    which norm catches its fault.
"""
import pytest
import torch
import torch.nn.functional as F

import backward_refs as B
import forward_refs as R

F64 = torch.float64
F32 = torch.float32
AGREE = 1e-12
N_FAULT = 128
RAGGED = (2, 80, 112)


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


# ----------------------------------------------------------------------- (a) two derivations
@pytest.mark.parametrize("op", ["conv1", "conv2", "deconv1", "deconv2"])
def test_gdn_reference_matches_oracle(op):
    c = R.case(op, 128, (2, 16, 48))
    ref = R.reference(op, c)
    # oracle.gdn re-parametrises its raw arguments in their own dtype; the reference takes the fp32
    # effective parameters (what the packing kernel computes). Raw float64 parameters that give
    # exactly those: √(x_eff + pedestal), which is never below its bound.
    be, ge = B.effective_params(c["beta"], c["gamma"])
    raw_b, raw_g = (torch.sqrt(t + R.oracle.GDN_PEDESTAL) for t in (be, ge))
    got = R.oracle.gdn(ref["pre"], raw_b, raw_g, op.startswith("deconv"))
    assert rel(ref["out"], got) < AGREE


def test_bits_reference_matches_oracle():
    for N in (128, 192):
        c = R.case("conv3", N, (2, 16, 48))
        p64 = {"bitEstimator." + k: v.double() for k, v in c["rate"].items()}
        for z in (torch.round(R.conv3(c["x"], c["w"])), R.conv3(c["x"], c["w"]) + c["noise"].double()):
            total, _ = R.oracle.estimate_bits(z, p64)
            per = R.bits(z, c["rate"])
            assert per.shape == (2,)
            assert abs(per.sum().item() - total.item()) <= AGREE * total.item()


# -------------------------------------------------------------- (b) CPU fp32 against the bars
def _worse(fig, key, errs):
    cur = fig.setdefault(key, {})
    for n, v in errs.items():
        cur[n] = max(cur.get(n, 0.0), v)


def cpu_fp32_figures():
    """({bar key: {"global": worst[, "row": worst]}}, worst excusable fraction) of the fp32
    evaluation of every reference against its float64 evaluation, over forward_refs.SHAPES and
    N = 128, 192."""
    fig, frac = {}, 0.0
    for N in (128, 192):
        for shape in R.SHAPES:
            for op in R.OPS:
                c = R.case(op, N, shape)
                r64, r32 = R.reference(op, c), R.reference(op, c, F32)
                for k in r64:
                    _worse(fig, f"{op}.{k}", R.errors(f"{op}.{k}", r32[k], r64[k]))
                if op == "conv3":
                    y = r64["y"]
                    frac = max(frac, R.excusable(y).double().mean().item())
                    # the bit sums: fp32 and float64 of the same latent, ŷ and ỹ
                    for key, z in (("bits.round", torch.round(r32["y"])),
                                   ("bits.noise", r32["y"] + c["noise"])):
                        _worse(fig, key, B.errors(R.bits(z, c["rate"], F32), R.bits(z, c["rate"])))
                    _worse(fig, "conv3.y", R.errors("conv3.y", r32["y"] + c["noise"],
                                                    y + c["noise"].double()))
                if op == "deconv3":
                    for k in ("clipped", "recon"):
                        _worse(fig, "sse", B.errors(R.sse(r32[k], c["x_ref"], F32),
                                                    R.sse(r32[k], c["x_ref"])))
    return fig, frac


def test_cpu_fp32_within_bars():
    """torch's fp32 evaluation of each formula passes the comparator at the GPU tests' bars, and
    the recorded figures the bars are 4 × of still bound what this machine measures."""
    fig, frac = cpu_fp32_figures()
    for key in sorted(fig):
        print(f"cpu fp32 {key:18s} " + "  ".join(f"{n} {v:.2e}" for n, v in fig[key].items()),
              " bars", R.BARS[key])
    print(f"excusable latents: at most {frac:.2e} of the elements")
    bad = {k: (e, R.BARS[k]) for k, e in fig.items() if not B.within(e, R.BARS[k])}
    assert not bad, bad
    assert set(fig) == {k for k in R.BARS if "@" not in k}
    assert frac < R.EXCUSABLE_MAX
    # nothing exceeds a standing bar
    for k, b in R.BARS.items():
        assert all(v <= (R.METRIC_REL if k.startswith(("bits", "sse")) else R.REL) for v in b.values()), k


def test_fp32_rounding_flips_only_in_the_band():
    """round(fp32 y) differs from round(y_ref) only inside the excusable band."""
    for N in (128, 192):
        c = R.case("conv3", N, RAGGED)
        y64, y32 = R.conv3(c["x"], c["w"]), R.conv3(c["x"], c["w"], F32)
        diff = torch.round(y32).double() != torch.round(y64)
        assert not (diff & ~R.excusable(y64)).any()


# ------------------------------------------------------------------------ (c) planted faults
def caught(key, bad, ref):
    """The norms under which ``bad`` misses the bars of ``key`` (forms never get looser bars than
    the standing one, so a fault beyond REL is caught in every form)."""
    e = R.errors(key, bad, ref)
    return {n for n in e if not e[n] <= R.BARS[key][n]}, e


def test_fault_border_tap_dropped():
    """One border output pixel of a strided convolution computed without one of its taps (conv2's
    pre-activation and GDN output, conv3's y, conv1's pre-activation). Both norms catch it: a tap
    is 1/25 (1/81) of the pixel's products."""
    for op, pix, tap in (("conv2", (1, 0, 5), (2, 4)), ("conv3", (0, 4, 0), (3, 2)),
                         ("conv1", (1, 19, 27), (4, 1))):
        c = R.case(op, N_FAULT, RAGGED)
        x, w = c["x"].double(), c["w"].double()
        s = 4 if op == "conv1" else 2
        one = torch.zeros_like(w)
        one[:, :, tap[0], tap[1]] = w[:, :, tap[0], tap[1]]
        good = F.conv2d(x, w, None if op == "conv3" else c["b"].double(), stride=s, padding=s)
        bad = good.clone()
        b, i, j = pix
        bad[b, :, i, j] -= F.conv2d(x, one, stride=s, padding=s)[b, :, i, j]
        assert not torch.equal(bad, good)
        key = "conv3.y" if op == "conv3" else op + ".pre"
        norms, e = caught(key, bad, good)
        print(f"tap dropped, {key}: caught by {sorted(norms)} {e}")
        assert "row" in norms
        if op != "conv3":
            norms, e = caught(op + ".out", R.gdn(bad, c["beta"], c["gamma"], False),
                              R.gdn(good, c["beta"], c["gamma"], False))
            print(f"tap dropped, {op}.out: caught by {sorted(norms)} {e}")
            assert "row" in norms


def test_fault_stride_phase_taps_swapped():
    """Phase (1, 1) of a transposed convolution computed with two of its taps in the wrong order
    (deconv1 / deconv2: kh, kw ∈ {1, 3}; deconv3: kh ∈ {1, 5}). Both norms catch it."""
    for op in ("deconv2", "deconv3"):
        c = R.case(op, N_FAULT, RAGGED)
        x, w, b = c["x"].double(), c["w"].double(), c["b"].double()
        s, p, o, a, z = (2, 2, 1, 1, 3) if op == "deconv2" else (4, 4, 3, 1, 5)
        ws = w.clone()
        ws[:, :, [a, z], :] = w[:, :, [z, a], :]
        good = F.conv_transpose2d(x, w, b, stride=s, padding=p, output_padding=o)
        bad = good.clone()
        bad[:, :, 1::s, 1::s] = F.conv_transpose2d(x, ws, b, stride=s, padding=p,
                                                   output_padding=o)[:, :, 1::s, 1::s]
        assert torch.equal(bad[:, :, 0::s, :], good[:, :, 0::s, :]) and not torch.equal(bad, good)
        for key, f in ((op + ".pre", lambda t: t), (op + ".out", lambda t: R.gdn(t, c["beta"], c["gamma"], True))) \
                if op == "deconv2" else (("deconv3.recon", lambda t: t), ("deconv3.clipped", lambda t: t.clamp(0, 1))):
            norms, e = caught(key, f(bad), f(good))
            print(f"taps swapped, {key}: caught by {sorted(norms)} {e}")
            assert "row" in norms


def _smallest_row(t):
    m = t.abs().amax(1)
    return [int(q) for q in torch.unravel_index(m.flatten().argmin(), m.shape)]


def test_fault_pixel_row_off():
    """One pixel row off by 1e-3 of the tensor's maximum: both norms catch it. The same row off by
    one and a half row bars of its own maximum, at the tensor's smallest row (what a wrong scale or a lost
    low-order part in one pixel's epilogue gives): only the row norm catches it."""
    only_row = 0
    for op in R.OPS:
        c = R.case(op, N_FAULT, RAGGED)
        for k, t in R.reference(op, c).items():
            key = f"{op}.{k}"
            rows = R.rows_of(key, t)
            b, i, j = _smallest_row(rows)
            bad = rows.clone()
            bad[b, :, i, j] += 1e-3 * t.abs().max()
            e = B.errors(bad, rows, (1,))
            assert e["global"] > R.BARS[key]["global"] and e["row"] > R.BARS[key]["row"], (key, e)
            bad = rows.clone()
            bad[b, :, i, j] *= 1 + 1.5 * R.BARS[key]["row"]
            e = B.errors(bad, rows, (1,))
            print(f"pixel row scaled, {key}: {e} bars {R.BARS[key]}")
            assert e["row"] > R.BARS[key]["row"], (key, e)
            only_row += e["global"] <= R.BARS[key]["global"]
    assert only_row >= 6          # of the 11 outputs; the global norm does not see it


def test_fault_tile_column_in_neighbour():
    """The last column of one 16-column tile written into its neighbour's first column (a ragged
    store one element too far). Both norms catch it: the pixel holds another pixel's values."""
    for op in ("conv1", "deconv2"):
        c = R.case(op, N_FAULT, RAGGED)          # grids 20×28: tiles end at column 15
        for k, t in R.reference(op, c).items():
            bad = t.clone()
            bad[1, :, 3, 16] = t[1, :, 3, 15]
            norms, e = caught(f"{op}.{k}", bad, t)
            print(f"column in the neighbour, {op}.{k}: caught by {sorted(norms)} {e}")
            assert "row" in norms


def test_fault_channel_chunk_permuted():
    """One 8-channel chunk of one pixel with its channels rotated by one (a chunk-major store with
    a wrong lane map), at the tensor's smallest pixel. The row norm catches it."""
    for op in ("conv2", "deconv1", "conv3"):
        c = R.case(op, N_FAULT, RAGGED)
        for k, t in R.reference(op, c).items():
            b, i, j = _smallest_row(t)
            bad = t.clone()
            bad[b, 40:48, i, j] = t[b, 40:48, i, j].roll(1)
            norms, e = caught(f"{op}.{k}", bad, t)
            print(f"chunk permuted, {op}.{k}: caught by {sorted(norms)} {e}")
            assert "row" in norms


def test_fault_tile_missing_from_sum():
    """A per-image SSE or bit sum without one (ragged) tile of one image."""
    c = R.case("deconv3", N_FAULT, RAGGED)
    recon, clipped = R.deconv3(c["x"], c["w"], c["b"])
    for t in (recon, clipped):
        d = (t - c["x_ref"].double()) ** 2
        part = d.clone()
        part[1, :, 64:80, 96:112] = 0                    # the corner tile's pixels do not reach the sum
        e = B.errors(part.sum((1, 2, 3)), d.sum((1, 2, 3)))
        assert not B.within(e, R.BARS["sse"]), e
    c = R.case("conv3", N_FAULT, RAGGED)
    for key, z in (("bits.round", torch.round(R.conv3(c["x"], c["w"]))),
                   ("bits.noise", R.conv3(c["x"], c["w"]) + c["noise"].double())):
        p = {"bitEstimator." + k: v.double() for k, v in c["rate"].items()}
        eb = R.oracle.element_bits(z, p)
        part = eb.clone()
        part[1, 64:128, 0:5, 0:7] = 0                    # one 64-channel slice of the image's one tile
        e = B.errors(part.sum((1, 2, 3)), eb.sum((1, 2, 3)))
        assert not B.within(e, R.BARS[key]), e


if __name__ == "__main__":
    fig, frac = cpu_fp32_figures()
    for k, v in sorted(fig.items()):
        print(k, v)
    print("excusable", frac)
