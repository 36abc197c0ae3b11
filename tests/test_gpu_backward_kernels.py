"""Every backward kernel against a float64 reference of its own (tests/backward_refs.py), from
exact synthetic inputs, at the smallest grids where an 8×8 tile edge, a stride phase, a split
boundary or a column sum can go wrong.

The fused input-gradient kernels (bwd_deconv3_igdn, bwd_deconv_igdn, bwd_conv_gdn, bwd_deconv_rate)
run in their fp32, x6 (split gradient in, split γ) and x6-γ (fp32 contraction, split γ) forms; the
weight, bias and parameter gradients in their fp32 and x6 forms. Each comparison uses two norms
(backward_refs.errors): the project's global max|Δ| / max|ref| and the worst pixel row (or weight
tap), which a single wrong pixel cannot hide in. Beside the references the tests pin what must hold
exactly: merge_planes(split output) == fp32 output, a split-only run writes the same split bits,
and (without a rate term) the kernel is linear under a power-of-two scale of the gradient.

Bars (backward_refs.BARS): 4 × the error of torch's CPU fp32 evaluation of the same formula against
float64 over the same shapes (tests/test_backward_refs_cpu.py prints those figures), capped by the
standing bars 2e-5 (contraction outputs) and 1e-4 (sums over pixels). The rate-parameter gradients
of bwd_deconv_rate have the fp32 oracle as their definition and keep the standing 1e-4. The k5 s2
convolution outputs (g_prev of bwd_deconv_igdn, g_y of bwd_deconv_rate) keep the standing 2e-5: the
engine adds their 25·N products into a running fp32 accumulator, whose error is several times that
of torch's blocked CPU sum (backward_refs.RUNNING_SUM), and so does the column sum of that g_prev,
which adds those outputs; nothing else needed more than 4 ×.

Worst figures over all shapes and N = 128, 192 (global / per row or tap; GPU: MI355X, fp32 and x6
forms together; each test prints its own):

    output                      CPU fp32           bar                GPU
    bwd_deconv3_igdn g_prev     7.4e-7 / 1.1e-6    3.0e-6 / 4.4e-6    6.0e-7 / 1.1e-6
    bwd_deconv3_igdn dn         5.9e-7 / 1.2e-6    2.4e-6 / 4.8e-6    6.2e-7 / 1.1e-6
    bwd_deconv3_igdn Σg, Σdn    3.4e-7, 4.1e-7     1.4e-6, 1.6e-6     3.9e-7, 4.5e-7
    bwd_deconv_igdn g_prev      4.9e-7 / 9.3e-7    2e-5 / 2e-5        2.8e-6 / 4.1e-6
    bwd_deconv_igdn dn          8.3e-7 / 1.7e-6    3.3e-6 / 6.8e-6    3.2e-6 / 4.0e-6
    bwd_deconv_igdn Σg, Σdn     5.9e-7, 4.8e-7     2e-5, 1.9e-6       3.7e-6, 1.5e-6
    bwd_conv_gdn g_prev         6.8e-7 / 1.7e-6    2.7e-6 / 6.8e-6    1.5e-6 / 2.4e-6
    bwd_conv_gdn dn             1.4e-6 / 2.4e-6    5.6e-6 / 9.6e-6    1.4e-6 / 2.8e-6
    bwd_conv_gdn Σg, Σdn        4.7e-7, 9.8e-7     1.9e-6, 3.9e-6     1.2e-6, 9.3e-7
    bwd_deconv_rate g_y         5.3e-7 / 9.3e-7    2e-5 / 2e-5        3.8e-6 / 5.0e-6
    bwd_deconv_rate g_y + rate  5.3e-7 / 8.7e-7    2e-5 / 2e-5        3.7e-6 / 5.1e-6
    rate-parameter gradients    (the reference)    1e-4               1.3e-5
    wgrad_k5 (fp32, x6)         5.7e-7 / 6.3e-7    2.3e-6 / 2.5e-6    5.7e-7 / 6.3e-7
    wgrad_k9 (fp32, x6)         6.1e-7 / 6.8e-7    2.4e-6 / 2.7e-6    5.3e-7 / 6.8e-7
    gdn_wgrad fp32              5.8e-7             2.3e-6             5.8e-7
    bias_grad_nhwc, _nchw       1.7e-7, 1.2e-7     6.8e-7, 4.8e-7     2.9e-7, 1.3e-7
    grad_recon                  4.2e-8             1.7e-7             8.6e-8
    gdn_param_chain             3.4e-8             1.4e-7             3.4e-8
    rate_param_grad             2.3e-7             9.2e-7             1.6e-7
"""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import backward_refs as R
from iclr_17_compression_amd import kernels
from iclr_17_compression_amd._lib import call
from iclr_17_compression_amd.model import ImageCompressor

pytestmark = pytest.mark.gpu

SCALE = 2.0 ** -20
F64 = torch.float64


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def check(name, got, ref, key, dims=None):
    """Print the errors of ``got`` against ``ref`` under the norms of bar ``key``, then assert."""
    bars = R.BARS[key]
    errs = R.errors(got, ref, dims if "row" in bars else None)
    print(f"{name}: " + "  ".join(f"{n} {v:.2e} (bar {bars[n]:.1e})" for n, v in errs.items()))
    assert R.within(errs, bars), (name, errs, bars)


@pytest.fixture(scope="module", params=[128, 192])
def model(request, device):
    """The codec with backward_refs.state(N) and the packed operands of its backward kernels, built
    as tests/golden/gen_engine_digests.py builds them."""
    N = request.param
    net = ImageCompressor(out_channel_N=N)
    net.load_state_dict({k: v.clone() for k, v in R.state(N).items()})
    net = net.to(device).eval()
    enc, dec = net.Encoder, net.Decoder
    d3c, d2c, d1c = dec.packed_bwd(False)
    w3t, _ = enc.packed_bwd()
    ops = {"deconv3_igdn": SimpleNamespace(w=d3c, w_split=dec.packed_bwd(True)[0], gdn=dec.igdn2),
           "deconv_igdn": SimpleNamespace(w=d2c, gdn=dec.igdn1),
           "conv_gdn": SimpleNamespace(w=w3t, gdn=enc.gdn2)}
    for o in ops.values():
        o.p, o.px = o.gdn.effective_params_bwd(), o.gdn.effective_params_bwd_x6()
    return SimpleNamespace(N=N, net=net, ops=ops, d1c=d1c, rate=net.bitEstimator.packed(),
                           device=device)


@pytest.fixture(scope="module")
def refs():
    """The float64 references, each built once and shared by the forms that are checked against it:
    (kernel, N, shape, rate) → (case, reference outputs)."""
    memo = {}

    def get(kernel, N, shape, rate=False):
        key = (kernel, N, shape, rate)
        if key not in memo:
            case = R.fused_case(kernel, N, shape)
            memo[key] = (case, R.fused_reference(kernel, case, F64, rate))
        return memo[key]

    return get


# ------------------------------------------------------------------ the three GDN-backward kernels
def run_fused(m, kernel, form, g, saved, want_f32=True):
    """One launch: g the upstream gradient (NCHW image gradient for deconv3_igdn, else NHWC) →
    (g_prev | None, dn, Σ g_prev, Σ dn[, g_prev split])."""
    o = m.ops[kernel]
    x6 = {} if form == "fp32" else {"want_split": True, "g6": o.px[3], "g6t": o.px[4],
                                    "want_f32": want_f32}
    if kernel == "deconv3_igdn":
        if form == "x6":
            return kernels.bwd_deconv3_igdn(g, None, saved, *o.px[:3], w_split=o.w_split, **x6)
        return kernels.bwd_deconv3_igdn(g, o.w, saved, *o.px[:3], **x6)
    fn = kernels.bwd_deconv_igdn if kernel == "deconv_igdn" else kernels.bwd_conv_gdn
    if form == "x6":
        return fn(None, o.w, saved, *o.px[:3], g_split=kernels.split_planes(g), **x6)
    return fn(g, o.w, saved, *o.px[:3], **x6)


FUSED = [(k, s) for k, shapes in (("deconv3_igdn", R.IMAGE_SHAPES), ("deconv_igdn", R.GRID_SHAPES),
                                  ("conv_gdn", R.GRID_SHAPES)) for s in shapes]


@pytest.mark.parametrize("form", ["fp32", "x6", "x6g"])
@pytest.mark.parametrize("kernel,shape", FUSED, ids=lambda v: v if isinstance(v, str) else
                         "x".join(map(str, v)))
def test_fused_gdn_backward(model, refs, kernel, shape, form):
    m = model
    case, (g_ref, dn_ref) = refs(kernel, m.N, shape)
    g = case["g"].to(m.device) if kernel == "deconv3_igdn" else nhwc(case["g"]).to(m.device)
    saved = nhwc(case["saved"]).to(m.device)
    out = run_fused(m, kernel, form, g, saved)
    torch.cuda.synchronize()
    tag = f"{kernel}.{form} N={m.N} {shape}"
    check(tag + " g_prev", nchw(out[0]), g_ref, kernel + ".g", (1,))
    check(tag + " dn", nchw(out[1]), dn_ref, kernel + ".dn", (1,))
    check(tag + " Σg_prev", out[2], R.pixel_sum(g_ref), kernel + ".sum_g")
    check(tag + " Σdn", out[3], R.pixel_sum(dn_ref), kernel + ".sum_dn")
    if form != "fp32":
        # the split output is the fp32 output, and does not depend on the fp32 one being written
        assert torch.equal(kernels.merge_planes(out[4]), out[0]), tag
        only = run_fused(m, kernel, form, g, saved, want_f32=False)
        assert only[0] is None and torch.equal(only[4], out[4]), tag
        assert all(torch.equal(a, b) for a, b in zip(only[1:4], out[1:4])), tag
    # linear under a power-of-two scale: gradients of a training step are ~1e-7 of these
    small = run_fused(m, kernel, form, g * SCALE, saved)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(small[:4], out[:4])):
        assert torch.equal(a, b * SCALE), (tag, "linearity", i)
    if form != "fp32":
        assert torch.equal(kernels.merge_planes(small[4]), kernels.merge_planes(out[4]) * SCALE), tag


# ------------------------------------------------------------------------------ bwd_deconv_rate
@pytest.mark.parametrize("rate", [False, True], ids=["norate", "rate"])
@pytest.mark.parametrize("form", ["fp32", "x6"])
@pytest.mark.parametrize("shape", R.GRID_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bwd_deconv_rate(model, refs, shape, form, rate):
    m = model
    case, (g_ref, p_ref) = refs("deconv_rate", m.N, shape, rate)
    B, h, w = shape
    g = nhwc(case["g"]).to(m.device)

    def run(g):
        y = nhwc(case["y"]).to(m.device) if rate else None
        g_bpp = torch.tensor(case["g_bpp"], device=m.device) if rate else None
        args = (m.d1c, y, m.rate if rate else None, g_bpp, case["count"], h, w)
        if form == "x6":
            return kernels.bwd_deconv_rate(None, *args, g_split=kernels.split_planes(g),
                                           want_split=True)
        return kernels.bwd_deconv_rate(g, *args)

    out = run(g)
    torch.cuda.synchronize()
    tag = f"deconv_rate.{form}.{'rate' if rate else 'norate'} N={m.N} {shape}"
    check(tag + " g_y", nchw(out[0]), g_ref, "deconv_rate.g_rate" if rate else "deconv_rate.g", (1,))
    if form == "x6":
        assert torch.equal(kernels.merge_planes(out[2]), out[0]), tag
    if rate:
        assert out[1].shape == (B * ((h + 7) // 8) * ((w + 7) // 8), 11, m.N)
        got = kernels.rate_param_grads(out[1], m.net.bitEstimator.params_in_order())
        for name, a, b in zip(R.RATE_ORDER, got, p_ref):
            check(f"{tag} ∂{name}", a.reshape(-1), b.reshape(-1), "deconv_rate.params")
    else:
        assert out[1] is None
        small = run(g * SCALE)
        assert torch.equal(small[0], out[0] * SCALE), (tag, "linearity")
        if form == "x6":
            assert torch.equal(kernels.merge_planes(small[2]), out[0] * SCALE), tag


# ------------------------------------------------------------------------------ weight gradients
@pytest.mark.parametrize("x6", [False, True], ids=["fp32", "x6"])
@pytest.mark.parametrize("B,Ho,Wo", R.WGRAD_K5_SHAPES)
def test_wgrad_k5(model, B, Ho, Wo, x6):
    """P = 35: one ragged k-step; 512: two splits of the fp32 kernel; 1587: six ragged splits of
    both kernels."""
    N, dev = model.N, model.device
    G, X = R.wgrad_case(5, N, B, Ho, Wo)
    ref = R.wgrad_k5(G.double(), X)
    Gd, Xd = nhwc(G).to(dev), nhwc(X).to(dev)
    got = (kernels.wgrad_k5_x6(kernels.split_planes(Gd), kernels.split_planes(Xd)) if x6
           else kernels.wgrad_k5(Gd, Xd))
    check(f"wgrad_k5{'_x6' if x6 else ''} N={N} {(B, Ho, Wo)}", got, ref, "wgrad_k5", (0, 1))


@pytest.mark.parametrize("x6", [False, True], ids=["fp32", "x6"])
@pytest.mark.parametrize("M,B,Ho,Wo", R.WGRAD_K9_SHAPES)
def test_wgrad_k9(device, M, B, Ho, Wo, x6):
    """X in [0, 1], NCHW; (2, 33, 9) has ragged 8×8 tiles on both sides."""
    G, X = R.wgrad_case(9, M, B, Ho, Wo)
    ref = R.wgrad_k9(G.double(), X)
    Gd, Xd = nhwc(G).to(device), X.to(device)
    got = kernels.wgrad_k9_x6(kernels.split_planes(Gd), Xd) if x6 else kernels.wgrad_k9(Gd, Xd)
    check(f"wgrad_k9{'_x6' if x6 else ''} {(M, B, Ho, Wo)}", got, ref, "wgrad_k9", (0, 1))


@pytest.mark.parametrize("C,P", R.GDN_WGRAD_SHAPES)
def test_gdn_wgrad_fp32(device, C, P):
    dn, u = R.normal(25, (P, C)), R.normal(26, (P, C))
    got = kernels.gdn_wgrad(dn.to(device), u.to(device), x6=False)
    check(f"gdn_wgrad C={C} P={P}", got, R.gdn_wgrad(dn.double(), u), "gdn_wgrad")


# ------------------------------------------------------------------------- bias, ∂recon, chains
@pytest.mark.parametrize("C,P", R.BIAS_NHWC_SHAPES)
def test_bias_grad_nhwc(device, C, P):
    G = R.normal(27, (P, C))
    check(f"bias_grad_nhwc C={C} P={P}", kernels.bias_grad_nhwc(G.to(device)), G.double().sum(0),
          "bias_nhwc")


@pytest.mark.parametrize("B,C,HW", R.BIAS_NCHW_SHAPES)
def test_bias_grad_nchw(device, B, C, HW):
    """HW below, above and not a multiple of the 4096-element plane chunk; C below and above one
    64-column block of sum_rows."""
    G = R.normal(28, (B, C, HW))
    got = kernels.bias_grad_nchw(G.view(B, C, 1, HW).to(device))
    check(f"bias_grad_nchw {(B, C, HW)}", got, G.double().sum((0, 2)), "bias_nchw")


@pytest.mark.parametrize("terms", ["mse", "clip", "both"])
def test_grad_recon(device, terms):
    """recon below 0, inside (0, 1), above 1 and exactly 0 and 1: the clamp passes its gradient on
    the closed interval, as torch's does."""
    recon = R.uniform(11, (2, 3, 16, 16), -0.5, 1.5)
    recon.view(-1)[::7] = 0.0
    recon.view(-1)[3::7] = 1.0
    x, g_clip = R.uniform(12, (2, 3, 16, 16), 0.0, 1.0), R.normal(13, (2, 3, 16, 16))
    g_mse = 0.7 if terms != "clip" else None
    gc = g_clip if terms != "mse" else None
    ref = R.grad_recon(recon.double(), x, g_mse, gc)
    got = kernels.grad_recon(recon.to(device), x.to(device),
                             None if g_mse is None else torch.tensor(g_mse, device=device),
                             None if gc is None else gc.to(device))
    check(f"grad_recon {terms}", got, ref, "grad_recon")
    assert torch.equal(got.cpu() == 0, ref == 0)      # the clamp's mask, element for element


def test_gdn_param_chain(model):
    """From given ∂β_eff, ∂γ_eff of both signs, β and γ entries on both sides of their bounds."""
    C, dev = model.N, model.device
    gdn = model.net.Encoder.gdn1
    beta, gamma = gdn.beta.detach(), gdn.gamma.detach()
    dbe, dge = R.normal(3, (C,)), R.normal(4, (C, C))
    bb, gb, _ = gdn.bounds_f32()
    assert (beta < bb).any() and (gamma < gb).any()
    db, dg = torch.empty(C, device=dev), torch.empty(C, C, device=dev)
    p = kernels._p
    dbe_d, dge_d = dbe.to(dev), dge.to(dev)
    call("iclr17_gdn_param_chain", p(beta.contiguous()), p(gamma.contiguous()), p(dbe_d), p(dge_d),
         C, ctypes.c_float(bb), ctypes.c_float(gb), p(db), p(dg), kernels._stream(db))
    rb, rg = R.gdn_param_chain(beta.cpu(), gamma.cpu(), dbe.double(), dge.double(), bb, gb)
    check(f"gdn_param_chain C={C} ∂β", db, rb, "gdn_param_chain")
    check(f"gdn_param_chain C={C} ∂γ", dg, rg, "gdn_param_chain")
    assert torch.equal(db.cpu() == 0, rb == 0) and torch.equal(dg.cpu() == 0, rg == 0)


@pytest.mark.parametrize("T", R.RATE_T)
def test_rate_param_grad(model, T):
    """From given partials [T, 11, C]."""
    C, dev = model.N, model.device
    part = R.normal(5, (T, 11, C))
    got = kernels.rate_param_grads(part.to(dev), model.net.bitEstimator.params_in_order())
    ref = R.rate_param_grad(part.double(), R.rate_params(C))
    for name, a, b in zip(R.RATE_ORDER, got, ref):
        check(f"rate_param_grad T={T} C={C} ∂{name}", a.reshape(-1), b, "rate_param_grad")
