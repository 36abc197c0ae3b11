"""Every forward kernel against a float64 reference of its own (tests/forward_refs.py), from exact
synthetic inputs, at the smallest image shapes where a tile edge, a stride phase, an H / W mix-up or
a layout can go wrong: the fp32, x6 and h3 forms of conv1 + GDN1, conv2 + GDN2, conv3 (+ quantiser
and rate), deconv1 / deconv2 + IGDN and deconv3. (bf16 has a rounded-operand contract of its own,
tests/test_gpu_bf16.py.)

Each comparison uses two norms (backward_refs.errors): the project's global max|Δ| / max|ref| and
the worst pixel row (one pixel's channels; for the image the 48 values of the 4×4 block one
stride-4 position produces, forward_refs.image_rows), which a single wrong pixel cannot hide in.
An h3 kernel's reference takes what the kernel sees: the merged h3 planes of the input, widened to
float64. Beside the references the tests pin what must hold exactly at every shape: merge_planes(x6
output) == fp32 output; the h3 output == h3_planes(fp32 output) in both layouts; a run with any
subset of the outputs writes the same bits; an image's results do not depend on its batch; the
16-row tiles of the h3 engine (a batch large enough to flip h3_tile_rows) give each image the bits
of the 8-row ones; ŷ == rint(y); folded reductions equal reduce_partials; and no entry point of the
h3 engine (nor deconv3_x6) writes a byte outside its outputs (64 KiB guard bands either side).

Bars (forward_refs.BARS): 4 × the error of torch's CPU fp32 evaluation of the same formula against
float64 over the same shapes (tests/test_forward_refs_cpu.py prints those figures), capped by the
standing bars 2e-5 (activations) and 1e-5 (per-image bits and SSE). Two forms add all 25·N products
of an output into one running fp32 sum and take the standing 2e-5 through ``widen=``, with the
reason beside the bar: the plain fp32 ``conv3`` (no quantiser, so none of the per-tap sums) and the
pre-activation of conv2 on the h3 engine (no two-level sums there, unlike its conv3). Nothing else
needed more than 4 ×, and the bit sums stay far below the 2.5e-6 at which the fp32 oracle would
have to stand in as their definition: they are compared with float64.

Worst figures over all shapes and N = 128, 192 (global / per row; GPU: MI355X, the variants of a
form together, the 16-row-tile runs included; each test prints its own):

    output           CPU fp32           bar                GPU fp32           GPU x6             GPU h3
    conv1.pre        7.4e-7 / 1.1e-6    3.0e-6 / 4.4e-6    6.9e-7 / 1.1e-6    6.9e-7 / 1.1e-6    4.8e-7 / 8.5e-7
    conv1.out        8.9e-7 / 1.1e-6    3.6e-6 / 4.4e-6    6.5e-7 / 9.2e-7    6.5e-7 / 9.2e-7    5.1e-7 / 7.1e-7
    conv2.pre        5.3e-7 / 7.4e-7    2.1e-6 / 3.0e-6    3.2e-7 / 5.3e-7    3.0e-7 / 4.6e-7    1.8e-6 / 3.0e-6 (bar 2e-5)
    conv2.out        7.9e-7 / 1.1e-6    3.2e-6 / 4.4e-6    4.8e-7 / 6.6e-7    3.8e-7 / 5.2e-7    1.6e-6 / 2.5e-6
    conv3 y, ỹ       5.4e-7 / 7.5e-7    2.2e-6 / 3.0e-6    3.5e-7 / 5.2e-7    2.7e-7 / 4.0e-7    2.5e-7 / 3.8e-7
    conv3 y, plain   5.4e-7 / 7.5e-7    2e-5 / 2e-5        2.5e-6 / 3.6e-6
    deconv1.pre      7.0e-7 / 1.1e-6    2.8e-6 / 4.4e-6    1.6e-6 / 2.2e-6    8.2e-7 / 1.2e-6    6.0e-7 / 8.2e-7
    deconv1.out      9.1e-7 / 1.6e-6    3.6e-6 / 6.4e-6    2.3e-6 / 3.1e-6    1.2e-6 / 1.8e-6    7.9e-7 / 1.2e-6
    deconv2.pre      1.2e-6 / 2.0e-6    4.8e-6 / 8.0e-6    1.8e-6 / 2.4e-6    1.4e-6 / 2.1e-6    9.4e-7 / 1.5e-6
    deconv2.out      1.2e-6 / 2.0e-6    4.8e-6 / 8.0e-6    1.8e-6 / 2.7e-6    1.5e-6 / 2.5e-6    1.0e-6 / 1.5e-6
    deconv3 recon    1.5e-6 / 2.6e-6    6.0e-6 / 1.0e-5    1.5e-6 / 2.8e-6    1.3e-6 / 2.2e-6    8.4e-7 / 2.3e-6
    deconv3 clipped  1.6e-6 / 3.7e-6    6.4e-6 / 1.5e-5    1.5e-6 / 2.6e-6    1.5e-6 / 2.4e-6    9.0e-7 / 1.4e-6
    bits, ŷ          1.4e-7             5.6e-7             9.4e-8             9.4e-8             7.1e-8
    bits, ỹ          9.1e-8             3.6e-7             7.6e-8             7.4e-8             7.4e-8
    SSE              1.2e-7             4.8e-7             5.6e-8             1.1e-7             7.7e-8

The ``rtab`` lookup and the direct evaluation of the bits give the same figures. Latents that may
round the other way (forward_refs.excusable): at most 7e-5 of the elements; none differed outside
the band. No guard byte was written. Wall time of this file on one MI355X: 7 s (284 cases).
"""
import ctypes
import itertools
from types import SimpleNamespace

import pytest
import torch

import backward_refs as B
import forward_refs as R
from iclr_17_compression_amd import _lib, kernels
from iclr_17_compression_amd._lib import call
from iclr_17_compression_amd.model import ImageCompressor

pytestmark = pytest.mark.gpu

F64 = torch.float64
GUARD = 64 * 1024
PATTERN = 0xA5
p, stream = kernels._p, kernels._stream
ids = lambda v: v if isinstance(v, str) else "x".join(map(str, v))      # noqa: E731


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def planes_nhwc(t):
    """A chunk-major h3 / split tensor [P,B,N/c,h,w,c] → NHWC planes [P,B,h,w,N] (bit patterns)."""
    if t.dim() == 5:
        return t
    P, b, nc, h, w, c = t.shape
    return t.permute(0, 1, 3, 4, 2, 5).reshape(P, b, h, w, nc * c)


def merged_h3_f64(s):
    """What an h3 kernel reads from planes ``s``: (hi + lo·2^-11)/σ_a, NHWC, float64 on the CPU."""
    h = planes_nhwc(s).view(torch.float16).cpu().double()
    return (h[0] + h[1] * 2.0 ** -11) / kernels.H3_SIGMA_A


class Checker:
    """Collects a test's comparisons: prints every figure, fails at the end with all that missed."""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def close(self, name, got, ref, key, form=None):
        bars = R.bars(key, form)
        errs = R.errors(key, got, ref)
        print(f"{self.tag} {name} [{key}]: " +
              "  ".join(f"{n} {v:.2e} (bar {bars[n]:.1e})" for n, v in errs.items()))
        if not B.within(errs, bars):
            self.bad.append((name, errs, bars))

    def exact(self, name, cond):
        if not bool(cond):
            print(f"{self.tag} {name}: NOT EXACT")
            self.bad.append((name, "not bit-equal"))

    def same(self, name, a, b):
        self.exact(name, a.shape == b.shape and torch.equal(a, b))

    def done(self):
        assert not self.bad, (self.tag, self.bad)


@pytest.fixture(scope="module", params=[128, 192])
def model(request, device):
    """The codec with backward_refs.state(N) and the packed operands of every forward form."""
    N = request.param
    net = ImageCompressor(out_channel_N=N)
    net.load_state_dict({k: v.clone() for k, v in B.state(N).items()})
    net = net.to(device).eval()
    enc, dec = net.Encoder, net.Decoder
    w1, w2, w3, _, _ = enc.packed()
    d1, d2, d3, _, _ = dec.packed()
    w2h, w3h = enc.packed_h3()
    d1h, d2h, d3h = dec.packed_h3k()

    def layer(conv, gdn, w, wh, **kw):
        return SimpleNamespace(w=w, wh=wh, bias=conv.bias, p=gdn.effective_params(),
                               px=gdn.effective_params_x6(), ph=gdn.effective_params_h3(), **kw)

    L = {"conv1": layer(enc.conv1, enc.gdn1, w1, enc.packed_conv1_h3(), w_x6=enc.packed_conv1_x6()),
         "conv2": layer(enc.conv2, enc.gdn2, w2, w2h),
         "deconv1": layer(dec.deconv1, dec.igdn1, d1, d1h),
         "deconv2": layer(dec.deconv2, dec.igdn2, d2, d2h),
         "conv3": SimpleNamespace(w=w3, wh=w3h, w_split=enc.packed_w3_split()),
         "deconv3": SimpleNamespace(w=d3, wx6=dec.packed_x6(), wh=d3h, bias=dec.deconv3.bias)}
    return SimpleNamespace(N=N, net=net, L=L, rate=net.bitEstimator.packed(),
                           rtab=net.bitEstimator.rate_table(), device=device,
                           flag=kernels.h3_range_flag(device))


@pytest.fixture(scope="module")
def refs():
    """The float64 references, each built once and shared by the forms checked against it:
    (op, N, shape, h3 input) → (case, reference outputs). With ``xin`` (the float64 NCHW input an h3
    kernel sees, where the h3 form does not hold the case's input exactly) the reference is taken
    on it."""
    memo = {}

    def get(op, N, shape, xin=None):
        key = (op, N, shape, xin is not None)
        if key not in memo:
            c = R.case(op, N, shape)
            memo[key] = (c, R.reference(op, c, F64, xin))
        return memo[key]

    return get


def three(x):
    """A batch of three distinct valid inputs made of the case's images (flips keep the range and
    integrality of an input)."""
    return torch.cat([x[:1], x[-1:].flip(3), x[:1].flip(2)]).contiguous()


# --------------------------------------------------------------- conv + GDN, deconv + IGDN layers
FORMS = {"conv1": ("fp32", "x6", "x6g", "x6w", "h3"),
         "conv2": ("fp32", "x6", "h3"),
         "deconv1": ("fp32", "x6", "x6cm", "h3", "h3cm", "h3int"),
         "deconv2": ("fp32", "x6", "x6cm", "h3", "h3cm")}
H3_IN_CM = {"conv2": kernels.CONV_CM, "deconv1": kernels.DECONV_CM, "deconv2": kernels.DECONV_CM}
OUT_OF = {"want_f32": "out", "want_pre": "pre", "want_x6": "x6", "want_split": "x6", "want_h3": "h3"}


def flags_of(op, form):
    """(the want_* flags of the wrapper of this form, whether a combination is accepted)."""
    if form == "fp32":
        return ("want_pre",), lambda w: True
    if form.startswith("x6"):
        if op.startswith("deconv"):
            return ("want_split", "want_f32", "want_pre"), lambda w: w["want_split"] or w["want_f32"]
        return ("want_f32", "want_pre"), lambda w: True
    return (("want_f32", "want_h3", "want_x6", "want_pre"),
            lambda w: w["want_f32"] or w["want_h3"] or w["want_x6"])


def layer_input(op, form, xd):
    """The device operand of a layer from its fp32 input (the image NCHW, else NHWC)."""
    if op == "conv1" or form == "fp32":
        return xd
    if form.startswith("x6"):
        return kernels.split_planes(xd)
    return kernels.h3_planes(xd, cm=H3_IN_CM[op])


def run_layer(m, op, form, xin, **w):
    """One launch of ``op`` in ``form`` on the operand of ``layer_input`` → {"out", "pre", "x6",
    "h3"}; the want_* flags default to True."""
    L, N = m.L[op], m.N
    f32, pre, x6, h3, split = (w.get(k, True) for k in ("want_f32", "want_pre", "want_x6", "want_h3",
                                                        "want_split"))
    d = dict(out=None, pre=None, x6=None, h3=None)
    if form == "fp32":
        if op == "conv1":
            r = kernels.conv1_gdn(xin, L.w, L.bias, *L.p, N, want_pre=pre)
        elif op == "conv2":
            r = kernels.conv2_gdn(xin, L.w, L.bias, *L.p, want_pre=pre)
        else:
            r = kernels.deconv_igdn(xin, L.w, L.bias, *L.p, want_pre=pre)
        d["out"], d["pre"] = r if pre else (r, None)
    elif form.startswith("x6"):
        if form == "x6w":
            r = kernels.conv1x6_gdn(xin, L.w_x6, L.bias, L.px[0], L.px[2], N, want_f32=f32, want_pre=pre)
        elif op == "conv1":
            r = kernels.conv1_gdn_x6(xin, L.w, L.bias, L.px[0], L.px[1], N, want_f32=f32, want_pre=pre,
                                     g6=L.px[2] if form == "x6g" else None)
        elif op == "conv2":
            r = kernels.conv2_gdn_x6(xin, L.w, L.bias, *L.px, want_f32=f32, want_pre=pre)
        else:
            r = kernels.deconv_igdn_x6(xin, L.w, L.bias, *L.px, want_split=split, want_f32=f32,
                                       want_pre=pre, chunk_major=form == "x6cm")
        d["x6"], d["out"], d["pre"] = r
    else:
        kw = dict(want_f32=f32, want_h3=h3, want_x6=x6, want_pre=pre)
        if op == "conv1":
            r = kernels.conv1_gdn_h3(xin, L.wh, L.bias, *L.ph, N, **kw)
            r = r if len(r) == 4 else (*r, None, None)
        elif op == "conv2":
            r = kernels.conv2_gdn_h3(xin, L.wh, L.bias, *L.ph, **kw)
        else:
            r = kernels.deconv_igdn_h3(xin, L.wh, L.bias, *L.ph, chunk_major=form == "h3cm",
                                       int_in=form == "h3int", **kw)
        r = r if len(r) == 4 else (*r, None)
        d["h3"], d["out"], d["x6"], d["pre"] = r
    return d


def h3_out_cm(op, form):
    return kernels.CONV_CM if op.startswith("conv") else \
        kernels.DECONV3_CM if form == "h3cm" else kernels.DECONV_CM


def check_encodings(c, op, form, o):
    """The split and h3 outputs of a launch encode exactly its fp32 output."""
    if o["x6"] is not None:
        c.same("merge_planes(x6) == fp32", kernels.merge_planes(o["x6"]), o["out"])
    if o["h3"] is not None:
        c.same("h3 == h3_planes(fp32)", o["h3"], kernels.h3_planes(o["out"], cm=h3_out_cm(op, form)))


def xin_for_reference(op, form, operand):
    """The float64 NCHW input of the reference of an h3 launch, or None when the h3 form holds the
    case's input exactly (conv1 reads the fp32 image; deconv1's latent is an integer)."""
    if not form.startswith("h3") or op in ("conv1", "deconv1"):
        return None
    return nchw(merged_h3_f64(operand))


LAYER_CASES = [(op, form) for op in ("conv1", "conv2", "deconv1", "deconv2") for form in FORMS[op]]


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
@pytest.mark.parametrize("op,form", LAYER_CASES)
def test_layer(model, refs, op, form, shape):
    """A conv + GDN or deconv + IGDN layer in one form: the pre-activation and the output against
    float64 under both norms, then the exact pins (encodings, layouts, output subsets, batch)."""
    m = model
    case = R.case(op, m.N, shape)
    xd = (case["x"] if op == "conv1" else nhwc(case["x"])).to(m.device)
    m.flag.zero_()
    operand = layer_input(op, form, xd)
    case, ref = refs(op, m.N, shape, xin_for_reference(op, form, operand))
    full = run_layer(m, op, form, operand)
    torch.cuda.synchronize()
    c = Checker(f"{op}.{form} N={m.N} {shape}")
    c.close("pre", nchw(full["pre"]), ref["pre"], op + ".pre", form)
    c.close("out", nchw(full["out"]), ref["out"], op + ".out", form)
    check_encodings(c, op, form, full)
    if op == "deconv1" and form.startswith("h3"):
        assert operand[1].eq(0).all()          # an integer latent has no lo plane
    # the same planes in either layout, and the integer-input form, against the plain h3 run
    if form in ("h3cm", "h3int", "x6cm"):
        base = run_layer(m, op, form[:2], operand)
        for k in ("out", "pre"):
            c.same(f"{k} == {form[:2]}'s", full[k], base[k])
        c.same("the same x6 planes", planes_nhwc(full["x6"]), planes_nhwc(base["x6"]))
        if form != "x6cm":
            c.same("the same h3 planes", planes_nhwc(full["h3"]), planes_nhwc(base["h3"]))
    # every accepted subset of the outputs writes the bits of the all-outputs run
    names, ok = flags_of(op, form)
    for combo in itertools.product((False, True), repeat=len(names)):
        w = dict(zip(names, combo))
        if all(combo) or not ok(w):
            continue
        sub = run_layer(m, op, form, operand, **w)
        off = {OUT_OF[f] for f, on in w.items() if not on}
        for k, t in sub.items():
            if t is None:
                c.exact(f"{k} missing with {w}", k in off or full[k] is None)
            else:
                c.exact(f"{k} unwanted with {w}", k not in off)
                c.same(f"{k} with {w}", t, full[k])
    # image b of a batch of three equals the same image run alone
    x3 = three(xd)
    o3 = run_layer(m, op, form, layer_input(op, form, x3))
    for b in range(3):
        o1 = run_layer(m, op, form, layer_input(op, form, x3[b:b + 1].contiguous()))
        for k in ("out", "pre"):
            c.same(f"{k} of image {b} alone", o1[k][0], o3[k][b])
        for k in ("x6", "h3"):
            if o1[k] is not None:
                c.same(f"{k} of image {b} alone", o1[k][:, 0], o3[k][:, b])
    if form.startswith("h3"):
        c.exact("range flag clear", int(m.flag.item()) == 0)
    c.done()


TILE_ROWS = [("conv2", "h3", 1), ("deconv1", "h3", 4), ("deconv1", "h3int", 4), ("deconv2", "h3", 4),
             ("deconv2", "h3cm", 4)]


@pytest.mark.parametrize("op,form,phases", TILE_ROWS)
def test_h3_sixteen_row_tiles(model, refs, op, form, phases):
    """The two images of the 80×112 case repeated up to the smallest batch at which h3_tile_rows
    (csrc/engine_h3.hip) takes 16-row tiles: images 0 and 1 against the reference, every later
    image b bit-equal to image b % 2."""
    m = model
    shape = R.TILE_ROWS_SHAPE
    x = nhwc(R.case(op, m.N, shape)["x"]).to(m.device)
    gh, gw = (x.shape[1] // 2, x.shape[2] // 2) if op == "conv2" else x.shape[1:3]
    reps = R.tile_rows_batch(gh, gw, phases) // 2
    groups = phases * -(-gh // 16) * -(-gw // 16)
    # 16-row tiles here and at no smaller even batch; 8-row ones for the case itself
    assert 2 * reps * groups >= 256 > (2 * reps - 2) * groups >= 2 * groups
    m.flag.zero_()
    operand = layer_input(op, form, x.repeat(reps, 1, 1, 1))
    _, ref = refs(op, m.N, shape, xin_for_reference(op, form, operand[:, :2]))
    o = run_layer(m, op, form, operand)
    torch.cuda.synchronize()
    c = Checker(f"{op}.{form} 16-row tiles N={m.N} B={2 * reps}")
    c.close("pre", nchw(o["pre"][:2]), ref["pre"], op + ".pre", form)
    c.close("out", nchw(o["out"][:2]), ref["out"], op + ".out", form)
    for k in ("out", "pre"):
        t = o[k].view(reps, 2, *o[k].shape[1:])
        c.exact(f"{k}: image b == image b % 2", (t == t[:1]).all())
    for k in ("x6", "h3"):
        t = o[k].view(o[k].shape[0], reps, 2, *o[k].shape[2:])
        c.exact(f"{k}: image b == image b % 2", (t == t[:, :1]).all())
    # and the bits of the 8-row tiles the two images get on their own
    small = run_layer(m, op, form, operand[:, :2].contiguous())
    for k in ("out", "pre"):
        c.same(f"{k} == the 8-row run's", o[k][:2], small[k])
    for k in ("x6", "h3"):
        c.same(f"{k} == the 8-row run's", o[k][:, :2], small[k])
    c.exact("range flag clear", int(m.flag.item()) == 0)
    c.done()


# ------------------------------------------------------------------------------------- conv3
def run_conv3(m, form, operand, noise=None, rtab=None, want_h3=True):
    """→ (ŷ or ỹ, bit partials, y, encoded ŷ | None), NHWC."""
    L = m.L["conv3"]
    if form == "fp32":
        return (*kernels.conv3_quant_rate(operand, L.w, m.rate, noise, want_y=True, rtab=rtab), None)
    if form.startswith("x6"):
        return kernels.conv3_quant_rate_x6(operand, L.w, m.rate, noise, want_y=True, rtab=rtab,
                                           w_split=L.w_split if form == "x6w" else None)
    return kernels.conv3_quant_rate_h3(operand, L.wh, m.rate, noise, want_y=True, rtab=rtab,
                                       want_h3=want_h3)


def conv3_operand(form, xd):
    return xd if form == "fp32" else kernels.split_planes(xd) if form.startswith("x6") else \
        kernels.h3_planes(xd, cm=kernels.CONV_CM)


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
@pytest.mark.parametrize("form", ["fp32", "x6", "x6w", "h3"])
def test_conv3_quant_rate(model, refs, form, shape):
    """conv3 with its quantiser and rate epilogue: round mode (bits evaluated and by ``rtab``
    lookup) and noise mode. The plain fp32 ``conv3`` rides with the fp32 form."""
    m = model
    case = R.case("conv3", m.N, shape)
    xd = nhwc(case["x"]).to(m.device)
    m.flag.zero_()
    operand = conv3_operand(form, xd)
    case, ref = refs("conv3", m.N, shape, nchw(merged_h3_f64(operand)) if form == "h3" else None)
    y_ref = ref["y"]
    noise = case["noise"].to(m.device)
    c = Checker(f"conv3.{form} N={m.N} {shape}")
    if form == "fp32":
        c.close("conv3 y", nchw(kernels.conv3(xd, m.L["conv3"].w)), y_ref, "conv3.y", "plain")
    ok = R.excusable(y_ref)
    assert ok.double().mean().item() < R.EXCUSABLE_MAX
    runs = {}
    for mode, nz, rtab in (("round", None, None), ("rtab", None, m.rtab), ("noise", noise, None)):
        z, part, y, enc = runs[mode] = run_conv3(m, form, operand, nz, rtab)
        torch.cuda.synchronize()
        c.close(f"{mode} y", nchw(y), y_ref, "conv3.y", form)
        zc = nchw(z).cpu().double()
        if nz is None:
            c.exact(f"{mode} ŷ == rint(y)", torch.equal(z, torch.round(y)))
            wrong = (zc != torch.round(y_ref)) & ~ok
            c.exact(f"{mode} ŷ == round(y_ref) outside the band ({int(wrong.sum())} differ)",
                    not wrong.any())
        else:
            c.close("ỹ", zc, y_ref + case["noise"].double(), "conv3.y", form)
        per, _ = kernels.reduce_partials(part)
        c.close(f"{mode} bits", per, R.bits(zc, case["rate"]),
                "bits.noise" if nz is not None else "bits.round", form)
        if form.startswith("x6"):
            c.same(f"{mode} merge_planes(split) == ŷ", kernels.merge_planes(enc), z)
        if form == "h3":
            c.same(f"{mode} h3 == h3_planes(ŷ)", enc, kernels.h3_planes(z, cm=kernels.DECONV_CM))
            sub = run_conv3(m, form, operand, nz, rtab, want_h3=False)
            c.exact(f"{mode} without the h3 output", sub[3] is None and
                    all(torch.equal(a, b_) for a, b_ in zip(sub[:3], (z, part, y))))
    c.same("rtab ŷ == evaluated ŷ", runs["rtab"][0], runs["round"][0])
    # image b of a batch of three equals the same image run alone (round mode; the partials too)
    x3 = three(xd)
    o3 = run_conv3(m, form, conv3_operand(form, x3))
    for b in range(3):
        o1 = run_conv3(m, form, conv3_operand(form, x3[b:b + 1].contiguous()))
        for k, name in enumerate(("ŷ", "partials", "y")):
            c.same(f"{name} of image {b} alone", o1[k][0], o3[k][b])
        if o1[3] is not None:
            c.same(f"encoded ŷ of image {b} alone", o1[3][:, 0], o3[3][:, b])
    if form == "h3":
        c.exact("range flag clear", int(m.flag.item()) == 0)
    c.done()


# ----------------------------------------------------------------------------------- deconv3
def cm32(planes):
    """NHWC planes [P,B,h,w,N] → chunk-major [P,B,N/32,h,w,32]."""
    P, b, h, w, N = planes.shape
    return planes.reshape(P, b, h, w, N // 32, 32).permute(0, 1, 4, 2, 3, 5).contiguous()


def deconv3_operand(form, xd):
    if form == "fp32":
        return xd
    if form.startswith("x6"):
        s = kernels.split_planes(xd)
        return cm32(s) if form == "x6cm" else s
    return kernels.h3_planes(xd, cm=kernels.DECONV3_CM)


def run_deconv3(m, form, operand, **kw):
    L = m.L["deconv3"]
    if form == "fp32":
        return kernels.deconv3(operand, L.w, L.bias, **kw)
    if form.startswith("x6"):
        return kernels.deconv3_x6(operand, L.wx6, L.bias, **kw)
    return kernels.deconv3_h3(operand, L.wh, L.bias, **kw)


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
@pytest.mark.parametrize("form", ["fp32", "x6", "x6cm", "h3"])
def test_deconv3(model, refs, form, shape):
    m = model
    b, H, W = shape
    case = R.case("deconv3", m.N, shape)
    xd = nhwc(case["x"]).to(m.device)
    x_ref = case["x_ref"].to(m.device)
    m.flag.zero_()
    operand = deconv3_operand(form, xd)
    case, ref = refs("deconv3", m.N, shape, nchw(merged_h3_f64(operand)) if form == "h3" else None)
    c = Checker(f"deconv3.{form} N={m.N} {shape}")
    outs = {}
    for unclipped in (False, True):
        clipped, recon, part = outs[unclipped] = run_deconv3(m, form, operand, x_ref=x_ref,
                                                             want_recon=True, sse_unclipped=unclipped)
        torch.cuda.synchronize()
        tag = "unclipped SSE" if unclipped else "clipped SSE"
        c.close(f"recon ({tag})", recon, ref["recon"], "deconv3.recon", form)
        c.close(f"clipped ({tag})", clipped, ref["clipped"], "deconv3.clipped", form)
        c.exact("the partials' shape", part.shape == (b, kernels.output_partials_per_image(H, W)))
        per, _ = kernels.reduce_partials(part)
        c.close(tag, per, R.sse((recon if unclipped else clipped).cpu(), case["x_ref"]), "sse", form)
    for k in range(2):
        c.same("the images do not depend on the SSE mode", outs[False][k], outs[True][k])
    clipped, recon, part = outs[False]
    c.exact("clipped == clamp(recon)", torch.equal(clipped, recon.clamp(0, 1)))
    # fewer outputs, the same bits
    sub = run_deconv3(m, form, operand)
    c.exact("clipped alone", sub[1] is None and sub[2] is None and torch.equal(sub[0], clipped))
    sub = run_deconv3(m, form, operand, x_ref=x_ref)
    c.exact("clipped and SSE", sub[1] is None and torch.equal(sub[0], clipped) and torch.equal(sub[2], part))
    # the folded bit reduction
    if form in ("x6cm", "h3"):
        bp = B.uniform(77, (b, 13), 0.0, 50.0).double().to(m.device)
        per_ref, tot_ref = kernels.reduce_partials(bp, 1.0 / 777.0)
        r = run_deconv3(m, form, operand, x_ref=x_ref, want_recon=True, bits=(bp, 1.0 / 777.0),
                        **({"bits_per_image": True} if form == "h3" else {}))
        c.exact("folded bits: images and SSE unchanged",
                all(torch.equal(a, b_) for a, b_ in zip(r[:3], (clipped, recon, part))))
        c.same("folded total == reduce_partials", r[3], tot_ref)
        if form == "h3":
            c.same("folded per-image bits == reduce_partials", r[4], per_ref)
    # image b of a batch of three equals the same image run alone
    x3, r3 = three(xd), three(x_ref)
    o3 = run_deconv3(m, form, deconv3_operand(form, x3), x_ref=r3, want_recon=True)
    for i in range(3):
        o1 = run_deconv3(m, form, deconv3_operand(form, x3[i:i + 1].contiguous()),
                         x_ref=r3[i:i + 1].contiguous(), want_recon=True)
        for k, name in enumerate(("clipped", "recon", "SSE partials")):
            c.same(f"{name} of image {i} alone", o1[k][0], o3[k][i])
    if form == "h3":
        c.exact("range flag clear", int(m.flag.item()) == 0)
    c.done()


# -------------------------------------------------------------------------------- guard bands
class Guarded:
    """Output buffers in the middle of larger allocations filled with a byte pattern: GUARD bytes
    either side of each. ``like(t)`` gives a tensor of t's shape and dtype to pass as an output;
    ``check`` reads the bands back."""

    def __init__(self, device):
        self.device, self.bufs = device, []

    def like(self, t):
        n = t.numel() * t.element_size()
        raw = torch.full((2 * GUARD + n,), PATTERN, dtype=torch.uint8, device=self.device)
        view = raw[GUARD:GUARD + n].view(t.dtype).view(t.shape)
        self.bufs.append((raw, n))
        return view

    def check(self, c):
        for i, (raw, n) in enumerate(self.bufs):
            c.exact(f"guard before output {i}", (raw[:GUARD] == PATTERN).all())
            c.exact(f"guard after output {i}", (raw[GUARD + n:] == PATTERN).all())


def guarded_call(c, m, name, outs, build_args):
    """Launch entry point ``name`` with every tensor of ``outs`` (the wrapper's results) replaced by
    a guarded buffer; the guards stay, the buffers hold the wrapper's bits."""
    g = Guarded(m.device)
    bufs = [g.like(t) for t in outs]
    torch.cuda.synchronize()
    call(name, *build_args(*bufs))
    torch.cuda.synchronize()
    g.check(c)
    for i, (a, b_) in enumerate(zip(bufs, outs)):
        c.same(f"{name} output {i} == the wrapper's", a, b_)


@pytest.mark.parametrize("shape", R.GUARD_SHAPES, ids=ids)
def test_guard_bands(model, shape):
    """The five h3 entry points and deconv3_x6 through the C ABI (the argument lists of
    kernels.py), all outputs wanted, every output pointer 64 KiB inside a patterned allocation: a
    ragged tile that stores past its grid would land in a guard. The test reads its own
    allocations only."""
    m = model
    N = m.N
    b, H, W = shape
    c = Checker(f"guard bands N={N} {shape}")
    flag = m.flag
    flag.zero_()
    # conv1 / conv2 + GDN
    for op in ("conv1", "conv2"):
        case = R.case(op, N, shape)
        xd = (case["x"] if op == "conv1" else nhwc(case["x"])).to(m.device)
        operand = layer_input(op, "h3", xd)
        L = m.L[op]
        o = run_layer(m, op, "h3", operand)
        guarded_call(c, m, f"iclr17_analysis_{op}_gdn_h3", [o["out"], o["pre"], o["h3"], o["x6"]],
                     lambda out, pre, h3, x6: (p(operand), b, H, W, N, p(L.wh), p(L.bias), p(L.ph[0]),
                                               p(L.ph[1]), p(out), p(pre), p(h3), kernels.CONV_CM,
                                               p(x6), p(flag), stream(operand)))
    # conv3 + quantiser + rate, both modes
    case = R.case("conv3", N, shape)
    operand = conv3_operand("h3", nhwc(case["x"]).to(m.device))
    L = m.L["conv3"]
    for mode, nz, rtab in ((_lib.ICLR17_QUANT_ROUND, None, m.rtab),
                           (_lib.ICLR17_QUANT_NOISE, case["noise"].to(m.device), None)):
        z, part, y, enc = run_conv3(m, "h3", operand, nz, rtab)
        guarded_call(c, m, "iclr17_analysis_conv3_quant_rate_h3", [y, z, enc, part],
                     lambda y_, z_, enc_, part_: (p(operand), b, H, W, N, p(L.wh), mode, p(nz),
                                                  p(m.rate), p(rtab), p(y_), p(z_), p(enc_),
                                                  kernels.DECONV_CM, p(part_), p(flag), stream(operand)))
    # deconv1 / deconv2 + IGDN, both output layouts, and the integer-input form
    for op, form in (("deconv1", "h3"), ("deconv1", "h3int"), ("deconv2", "h3"), ("deconv2", "h3cm")):
        operand = layer_input(op, form, nhwc(R.case(op, N, shape)["x"]).to(m.device))
        L = m.L[op]
        o = run_layer(m, op, form, operand)
        hh, ww = operand.shape[3], operand.shape[4]
        guarded_call(c, m, "iclr17_synthesis_deconv_igdn_h3", [o["out"], o["pre"], o["h3"], o["x6"]],
                     lambda out, pre, h3, x6: (p(operand), b, hh, ww, N, p(L.wh), p(L.bias), p(L.ph[0]),
                                               p(L.ph[1]), p(out), p(pre), p(h3), p(x6),
                                               h3_out_cm(op, form), int(form == "h3int"), p(flag),
                                               stream(operand)))
    # deconv3: h3, and x6 in both input forms
    case = R.case("deconv3", N, shape)
    xd, x_ref = nhwc(case["x"]).to(m.device), case["x_ref"].to(m.device)
    L = m.L["deconv3"]
    bp = B.uniform(77, (b, 13), 0.0, 50.0).double().to(m.device)
    scale = ctypes.c_double(1.0 / 777.0)
    for unclipped in (0, 1):
        operand = deconv3_operand("h3", xd)
        r = run_deconv3(m, "h3", operand, x_ref=x_ref, want_recon=True, sse_unclipped=bool(unclipped),
                        bits=(bp, 1.0 / 777.0), bits_per_image=True)
        guarded_call(c, m, "iclr17_synthesis_deconv3_h3", list(r),
                     lambda cl, rc, part, tot, per: (p(operand), b, H, W, N, p(L.wh), p(L.bias), p(x_ref),
                                                     p(cl), p(rc), p(part), unclipped, p(bp), bp.shape[1],
                                                     p(per), p(tot), scale, p(flag), stream(operand)))
        operand = deconv3_operand("x6cm", xd)
        r = run_deconv3(m, "x6cm", operand, x_ref=x_ref, want_recon=True, sse_unclipped=bool(unclipped),
                        bits=(bp, 1.0 / 777.0))
        guarded_call(c, m, "iclr17_synthesis_deconv3_x6_cm_bits", list(r),
                     lambda cl, rc, part, tot: (p(operand), b, H, W, N, p(L.wx6), p(L.bias), p(x_ref),
                                                p(cl), p(rc), p(part), unclipped, p(bp), bp.shape[1],
                                                None, p(tot), scale, stream(operand)))
        operand = deconv3_operand("x6", xd)
        r = run_deconv3(m, "x6", operand, x_ref=x_ref, want_recon=True, sse_unclipped=bool(unclipped))
        guarded_call(c, m, "iclr17_synthesis_deconv3_x6", list(r),
                     lambda cl, rc, part: (p(operand), b, H, W, N, p(L.wx6), p(L.bias), p(x_ref),
                                           p(cl), p(rc), p(part), unclipped, stream(operand)))
    c.exact("range flag clear", int(flag.item()) == 0)
    c.done()
