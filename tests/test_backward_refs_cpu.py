"""The backward-kernel references and their comparator, checked on the CPU (tests/backward_refs.py):

(a) every explicit float64 helper against float64 autograd through F.conv2d / F.conv_transpose2d
    and the GDN formula: two independent derivations, equal to 1e-12;
(b) the same formulas evaluated by torch in fp32 pass the comparator at the bars the GPU tests
    use, at every shape those tests run (the bars are 4 × these figures, see backward_refs.BARS);
(c) planted faults on the reference do not pass it at those bars: a pixel row off by 1e-3, a border
    pixel with one tap dropped, a stride phase with its taps swapped, a tile missing from a column
    sum, a split-K slice missing from a weight gradient.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import backward_refs as R

F64 = torch.float64
AGREE = 1e-12


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def leaf(t):
    return t.detach().double().clone().requires_grad_(True)


# ----------------------------------------------------------------------- (a) two derivations
def _gdn_forward(x, be, ge, inverse):
    n = F.conv2d(x * x, ge.view(*ge.shape, 1, 1), be)          # GDN.py:83
    return x * torch.sqrt(n) if inverse else x / torch.sqrt(n)


@pytest.mark.parametrize("kernel,shape", [("deconv3_igdn", (2, 32, 48)), ("deconv_igdn", (2, 5, 7)),
                                          ("conv_gdn", (2, 5, 7)), ("deconv_rate", (2, 5, 7))])
def test_fused_helpers_match_autograd(kernel, shape):
    """∂(Σ forward(saved)·g)/∂saved by autograd through the layer's forward (IGDN then the
    transposed convolution, GDN then the convolution) equals the helper's explicit g_prev; dn
    equals autograd's gradient with respect to the norm pool n."""
    N = 128
    c = R.fused_case(kernel, N, shape)
    g = c["g"].double()
    got = R.fused_reference(kernel, c)
    if kernel == "deconv_rate":
        y = leaf(torch.zeros(shape[0], N, shape[1], shape[2]))
        v = F.conv_transpose2d(y, c["w"].double(), stride=2, padding=2, output_padding=1)
        (v * g).sum().backward()
        assert rel(got[0], y.grad) < AGREE
        return
    be, ge = R.effective_params(c["beta"], c["gamma"])
    x = leaf(c["saved"])
    n = (be.view(1, -1, 1, 1) + F.conv2d(x * x, ge.view(N, N, 1, 1))).requires_grad_(True)
    n.retain_grad()
    w = c["w"].double()
    if kernel == "conv_gdn":
        out = F.conv2d(x / torch.sqrt(n), w, stride=2, padding=2)
    else:
        s, op = (4, 3) if kernel == "deconv3_igdn" else (2, 1)
        out = F.conv_transpose2d(x * torch.sqrt(n), w, stride=s, padding=(w.shape[2] - 1) // 2,
                                 output_padding=op)
    assert out.shape == g.shape
    (out * g).sum().backward()
    assert rel(got[0], x.grad) < AGREE
    assert rel(got[1], n.grad) < AGREE
    # and the plain module formula (n not a leaf) gives the same ∂saved
    x2 = leaf(c["saved"])
    a = _gdn_forward(x2, be, ge, kernel != "conv_gdn")
    out2 = (F.conv2d(a, w, stride=2, padding=2) if kernel == "conv_gdn" else
            F.conv_transpose2d(a, w, stride=s, padding=(w.shape[2] - 1) // 2, output_padding=op))
    (out2 * g).sum().backward()
    assert rel(got[0], x2.grad) < AGREE


@pytest.mark.parametrize("kind,M,B,Ho,Wo", [(5, 128, 2, 5, 7), (9, 128, 2, 5, 3)])
def test_wgrad_helper_matches_conv2d_weight(kind, M, B, Ho, Wo):
    G, X = (t.double() for t in R.wgrad_case(kind, M, B, Ho, Wo))
    k, s, p = (5, 2, 2) if kind == 5 else (9, 4, 4)
    ref = torch.nn.grad.conv2d_weight(X, (M, X.shape[1], k, k), G, stride=s, padding=p)
    got = R.wgrad_k5(G, X) if kind == 5 else R.wgrad_k9(G, X)
    assert rel(got, ref) < AGREE
    w = leaf(torch.zeros(M, X.shape[1], k, k))
    (F.conv2d(X, w, stride=s, padding=p) * G).sum().backward()
    assert rel(got, w.grad) < AGREE


def test_parameter_helpers_match_autograd():
    C = 128
    sd = R.state(C)
    beta, gamma = sd["Encoder.gdn1.beta"], sd["Encoder.gdn1.gamma"]
    # dγ_eff, Σ over pixels
    dn, u = R.normal(1, (50, C)).double(), R.normal(2, (50, C)).double()
    ge = leaf(torch.zeros(C, C))
    ((u * u) @ ge.t() * dn).sum().backward()
    assert rel(R.gdn_wgrad(dn, u), ge.grad) < AGREE
    # the reparametrisation chain, gradients of both signs on entries on both sides of the bound
    bb, gb = float(torch.tensor(oracle_bound("beta")).float()), float(torch.tensor(oracle_bound("gamma")).float())
    dbe, dge = R.normal(3, (C,)).double(), R.normal(4, (C, C)).double()
    b, g = leaf(beta), leaf(gamma)
    be = R.oracle.lower_bound(b, bb) ** 2 - R.oracle.GDN_PEDESTAL
    gg = R.oracle.lower_bound(g, gb) ** 2 - R.oracle.GDN_PEDESTAL
    ((be * dbe).sum() + (gg * dge).sum()).backward()
    db, dg = R.gdn_param_chain(beta, gamma, dbe, dge, bb, gb)
    assert (beta < bb).any() and (gamma < gb).any()
    assert rel(db, b.grad) < AGREE and rel(dg, g.grad) < AGREE
    assert ((db == 0) == (b.grad == 0)).all() and ((dg == 0) == (g.grad == 0)).all()
    # the rate parameters' chain
    rp = R.rate_params(C)
    part = R.normal(5, (7, 11, C)).double()
    leaves = {k: leaf(v) for k, v in rp.items()}
    S = part.sum(0)
    sum(((F.softplus(leaves[k]) if k[-1] == "h" else leaves[k] if k[-1] == "b"
          else torch.tanh(leaves[k])).reshape(-1) * S[i]).sum()
        for i, k in enumerate(R.RATE_ORDER)).backward()
    for got, k in zip(R.rate_param_grad(part, rp), R.RATE_ORDER):
        assert rel(got, leaves[k].grad.reshape(-1)) < AGREE, k
    # ∂recon of the two loss terms, recon on every side of the clamp and on its ends
    recon, x, g_clip = recon_case()
    for g_mse, gc in ((0.7, None), (None, g_clip), (0.7, g_clip)):
        r = leaf(recon)
        loss = 0
        if g_mse is not None:
            loss = loss + g_mse * torch.mean((r - x.double()) ** 2)
        if gc is not None:
            loss = loss + (r.clamp(0, 1) * gc.double()).sum()
        loss.backward()
        got = R.grad_recon(recon.double(), x, g_mse, gc)
        assert (got - r.grad).abs().max() <= AGREE * r.grad.abs().max()


def oracle_bound(which):
    return R.oracle.GDN_BETA_BOUND if which == "beta" else R.oracle.GDN_GAMMA_BOUND


def recon_case():
    """(recon, x, g_clip) NCHW [2,3,16,16]: recon below 0, inside (0, 1), above 1, exactly 0 and 1."""
    recon = R.uniform(11, (2, 3, 16, 16), -0.5, 1.5)
    recon.view(-1)[::7] = 0.0
    recon.view(-1)[3::7] = 1.0
    assert all(m.any() for m in (recon < 0, (recon > 0) & (recon < 1), recon > 1, recon == 0, recon == 1))
    return recon, R.uniform(12, (2, 3, 16, 16), 0.0, 1.0), R.normal(13, (2, 3, 16, 16))


# -------------------------------------------------------------- (b) CPU fp32 against the bars
def _worse(fig, key, errs):
    cur = fig.setdefault(key, {})
    for n, v in errs.items():
        cur[n] = max(cur.get(n, 0.0), v)


def cpu_fp32_figures():
    """{bar key: {"global": worst[, "row": worst]}} of the fp32 evaluation of every reference
    against its float64 evaluation, over the shapes of the GPU tests and N = 128, 192."""
    fig = {}
    f32 = torch.float32
    for N in (128, 192):
        for kernel, shapes in (("deconv3_igdn", R.IMAGE_SHAPES), ("deconv_igdn", R.GRID_SHAPES),
                               ("conv_gdn", R.GRID_SHAPES)):
            for shape in shapes:
                c = R.fused_case(kernel, N, shape)
                (g64, dn64), (g32, dn32) = R.fused_reference(kernel, c), R.fused_reference(kernel, c, f32)
                _worse(fig, kernel + ".g", R.errors(g32, g64, (1,)))
                _worse(fig, kernel + ".dn", R.errors(dn32, dn64, (1,)))
                _worse(fig, kernel + ".sum_g", R.errors(R.pixel_sum(g32), R.pixel_sum(g64)))
                _worse(fig, kernel + ".sum_dn", R.errors(R.pixel_sum(dn32), R.pixel_sum(dn64)))
        for shape in R.GRID_SHAPES:
            c = R.fused_case("deconv_rate", N, shape)
            for rate in (False, True):
                g64, _ = R.fused_reference("deconv_rate", c, F64, rate)
                g32, _ = R.fused_reference("deconv_rate", c, f32, rate)
                _worse(fig, "deconv_rate.g_rate" if rate else "deconv_rate.g", R.errors(g32, g64, (1,)))
        for B, Ho, Wo in R.WGRAD_K5_SHAPES:
            G, X = R.wgrad_case(5, N, B, Ho, Wo)
            _worse(fig, "wgrad_k5", R.errors(R.wgrad_k5(G, X), R.wgrad_k5(G.double(), X), (0, 1)))
    for M, B, Ho, Wo in R.WGRAD_K9_SHAPES:
        G, X = R.wgrad_case(9, M, B, Ho, Wo)
        _worse(fig, "wgrad_k9", R.errors(R.wgrad_k9(G, X), R.wgrad_k9(G.double(), X), (0, 1)))
    for C, P in R.GDN_WGRAD_SHAPES:
        dn, u = R.normal(25, (P, C)), R.normal(26, (P, C))
        _worse(fig, "gdn_wgrad", R.errors(R.gdn_wgrad(dn, u), R.gdn_wgrad(dn.double(), u)))
    for C, P in R.BIAS_NHWC_SHAPES:
        G = R.normal(27, (P, C))
        _worse(fig, "bias_nhwc", R.errors(G.sum(0), G.double().sum(0)))
    for B, C, HW in R.BIAS_NCHW_SHAPES:
        G = R.normal(28, (B, C, HW))
        _worse(fig, "bias_nchw", R.errors(G.sum((0, 2)), G.double().sum((0, 2))))
    recon, x, g_clip = recon_case()
    _worse(fig, "grad_recon", R.errors(R.grad_recon(recon, x, 0.7, g_clip),
                                       R.grad_recon(recon.double(), x, 0.7, g_clip)))
    for C in (128, 192):
        sd = R.state(C)
        beta, gamma = sd["Encoder.gdn1.beta"], sd["Encoder.gdn1.gamma"]
        dbe, dge = R.normal(3, (C,)), R.normal(4, (C, C))
        bb, gb = (float(torch.tensor(oracle_bound(k)).float()) for k in ("beta", "gamma"))
        for a32, a64 in zip(R.gdn_param_chain(beta, gamma, dbe, dge, bb, gb),
                            R.gdn_param_chain(beta, gamma, dbe.double(), dge.double(), bb, gb)):
            _worse(fig, "gdn_param_chain", R.errors(a32, a64))
        for T in R.RATE_T:
            part = R.normal(5, (T, 11, C))
            for a32, a64 in zip(R.rate_param_grad(part, R.rate_params(C)),
                                R.rate_param_grad(part.double(), R.rate_params(C))):
                _worse(fig, "rate_param_grad", R.errors(a32, a64))
    return fig


def test_cpu_fp32_within_bars():
    """torch's fp32 evaluation of each formula passes the comparator at the GPU tests' bars, and
    the recorded figures the bars are 4 × of still bound what this machine measures."""
    fig = cpu_fp32_figures()
    for key in sorted(fig):
        print(f"cpu fp32 {key:24s} " + "  ".join(f"{n} {v:.2e}" for n, v in fig[key].items()),
              " bars", R.BARS[key])
    bad = {k: (e, R.BARS[k]) for k, e in fig.items() if not R.within(e, R.BARS[k])}
    assert not bad, bad
    assert set(fig) <= set(R.BARS)


# ------------------------------------------------------------------------ (c) planted faults
N_FAULT = 128


def test_fault_pixel_row_scaled():
    """One pixel row (all channels of one pixel) times 1 + 1e-3, at the pixel where the global
    norm sees it least (the smallest row of the tensor)."""
    for kernel, shape in (("deconv_igdn", (3, 9, 17)), ("conv_gdn", (3, 9, 17)),
                          ("deconv3_igdn", (2, 48, 80))):
        ref, dn = R.fused_reference(kernel, R.fused_case(kernel, N_FAULT, shape))
        for t, key in ((ref, kernel + ".g"), (dn, kernel + ".dn")):
            bad = t.clone()
            flat = t.abs().amax(1).flatten()
            b, i, j = [int(q) for q in torch.unravel_index(flat.argmin(), t.abs().amax(1).shape)]
            bad[b, :, i, j] *= 1 + 1e-3
            e = R.errors(bad, t, (1,))
            assert e["row"] > 10 * R.BARS[key]["row"], (key, e)
            assert not R.within(e, R.BARS[key]), (key, e)


def test_fault_border_tap_dropped():
    """One border output pixel of the strided convolution computed without one of its taps."""
    c = R.fused_case("deconv_igdn", N_FAULT, (3, 9, 17))
    g, w = c["g"].double(), c["w"].double()
    be, ge = R.effective_params(c["beta"], c["gamma"])
    t = F.conv2d(g, w, stride=2, padding=2)
    one = torch.zeros_like(w)
    one[:, :, 2, 4] = w[:, :, 2, 4]                     # tap (kh, kw) = (2, 4), inside the image
    t_bad = t.clone()
    t_bad[1, :, 0, 5] -= F.conv2d(g, one, stride=2, padding=2)[1, :, 0, 5]
    good = R.igdn_backward(t, c["saved"].double(), be, ge)
    bad = R.igdn_backward(t_bad, c["saved"].double(), be, ge)
    for a, b_, key in ((bad[0], good[0], "deconv_igdn.g"), (bad[1], good[1], "deconv_igdn.dn")):
        assert not R.within(R.errors(a, b_, (1,)), R.BARS[key]), key
    # the plain convolution of bwd_deconv_rate
    assert not R.within(R.errors(t_bad, t, (1,)), R.BARS["deconv_rate.g"])


def test_fault_stride_phase_taps_swapped():
    """Phase (1, 1) of the transposed convolution (output rows and columns odd, taps kh, kw ∈
    {1, 3}) computed with its taps in the wrong order."""
    c = R.fused_case("conv_gdn", N_FAULT, (3, 9, 17))
    g, w = c["g"].double(), c["w"].double()
    be, ge = R.effective_params(c["beta"], c["gamma"])
    t = F.conv_transpose2d(g, w, stride=2, padding=2, output_padding=1)
    ws = w.clone()
    ws[:, :, [1, 3], :] = w[:, :, [3, 1], :]
    ws[:, :, :, [1, 3]] = ws[:, :, :, [3, 1]]
    t_bad = t.clone()
    t_bad[:, :, 1::2, 1::2] = F.conv_transpose2d(g, ws, stride=2, padding=2,
                                                 output_padding=1)[:, :, 1::2, 1::2]
    assert torch.equal(t_bad[:, :, 0::2, :], t[:, :, 0::2, :])
    good = R.gdn_backward(t, c["saved"].double(), be, ge)
    bad = R.gdn_backward(t_bad, c["saved"].double(), be, ge)
    for a, b_, key in ((bad[0], good[0], "conv_gdn.g"), (bad[1], good[1], "conv_gdn.dn")):
        assert not R.within(R.errors(a, b_, (1,)), R.BARS[key]), key


def test_fault_tile_missing_from_column_sum():
    """Σ over pixels without one 8×8 tile of one image, for both partial buffers of a kernel."""
    for kernel, shape, sl in (("deconv_igdn", (3, 9, 17), (slice(0, 8), slice(8, 16))),
                              ("conv_gdn", (3, 9, 17), (slice(16, 18), slice(32, 34))),
                              ("deconv3_igdn", (2, 48, 80), (slice(8, 12), slice(16, 20)))):
        for t, key in zip(R.fused_reference(kernel, R.fused_case(kernel, N_FAULT, shape)),
                          (kernel + ".sum_g", kernel + ".sum_dn")):
            part = t.clone()
            part[1, :, sl[0], sl[1]] = 0        # the (ragged) tile's pixels do not reach the sum
            e = R.errors(R.pixel_sum(part), R.pixel_sum(t))
            assert not R.within(e, R.BARS[key]), (key, e)


def test_fault_split_k_slice_missing():
    """A weight gradient without one of the six pixel slices of its split-K reduction (P = 1587)."""
    B, Ho, Wo = 3, 23, 23
    G, X = (t.double() for t in R.wgrad_case(5, N_FAULT, B, Ho, Wo))
    ref = R.wgrad_k5(G, X)
    P, per = B * Ho * Wo, math.ceil(B * Ho * Wo / 6)
    Gp = G.permute(0, 2, 3, 1).reshape(P, -1).clone()
    Gp[5 * per:] = 0                                   # the last, ragged slice
    bad = R.wgrad_k5(Gp.reshape(B, Ho, Wo, -1).permute(0, 3, 1, 2), X)
    e = R.errors(bad, ref, (0, 1))
    assert not R.within(e, R.BARS["wgrad_k5"]), e
    G9, X9 = (t.double() for t in R.wgrad_case(9, 192, 2, 33, 9))
    G9b = G9.clone()
    G9b[1, :, 32:, 8:] = 0                             # the ragged corner tile of the second image
    e = R.errors(R.wgrad_k9(G9b, X9), R.wgrad_k9(G9, X9), (0, 1))
    assert not R.within(e, R.BARS["wgrad_k9"]), e


if __name__ == "__main__":
    for k, v in sorted(cpu_fp32_figures().items()):
        print(k, v)
