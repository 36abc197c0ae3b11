"""Rate–distortion optimised quantisation on the GPU (csrc/rdoq.hip and the layers above it,
DESIGN.md §0j): the picks against the definition in float64, exact properties, the bit totals
against the existing rate kernels, the limits of lam, the codec round trip and the synthesis
gains. The weights are synthetic: nothing here is a statement about quality."""
import math

import numpy as np
import pytest
import torch

import rdo_refs as R
from iclr_17_compression_amd import codec, kernels, synth
from iclr_17_compression_amd.model import ImageCompressor
from oracle import codec_ref as oracle

pytestmark = pytest.mark.gpu

DELTAS = [codec.step_size(s) for s in range(codec.STEPS)]
MIXED = [(49, 83), (64, 96), (50, 96), (64, 81)]    # one canvas, 64×96 (test_gpu_ratectl.py)


def make_net(N, device):
    n = ImageCompressor(out_channel_N=N)
    n.load_state_dict({k: torch.from_numpy(v) for k, v in synth.trained_like_state_dict(N, 1).items()})
    return n.to(device).eval()


@pytest.fixture(scope="module")
def nets(device):
    made = {}

    def get(N):
        if N not in made:
            net = make_net(N, device)
            ims = R.images()
            with kernels.precision_scope("x6"):
                ys = [net.latents(R.batch(ims[:2]).to(device)), net.latents(R.batch(ims[2:]).to(device))]
            assert [tuple(y.shape) for y in ys] == [(2, 4, 6, N), (1, 1, 1, N)]
            made[N] = (net, net.bitEstimator.packed(), ys)
        return made[N]
    return get


def np_pack(pack):
    return pack.cpu().numpy().reshape(11, -1)


def lam_on(device, rdo, g):
    return torch.from_numpy(R.lam_of(rdo, g)).to(device)


def combos(N):
    for s in R.INDICES:
        for rdo in R.LAMBDAS:
            for kind in ("unit", "ramp") if rdo == 1.0 else ("unit",):
                yield s, rdo, kind, R.lam_of(rdo, R.weights(N, kind))


def rate_bits_of(y_hat, pack, N, d):
    """The existing kernels' per-image bits of ŷ at step d: float64 [B]."""
    sp = kernels.pack_rate_step(pack, N, d)
    return kernels.reduce_partials(kernels.rate_bits(y_hat.permute(0, 3, 1, 2), sp))[0]


def element_bits_gpu(y_hat, pack, N, d):
    """Per-element bits through the existing rate_bits kernel, exactly: channel c's elements as
    one-element images under channel c's column of the step pack (a partial is then the element's
    fp32 bits plus zeros). y_hat NHWC → float64 [B·h·w, N]."""
    sp = kernels.pack_rate_step(pack, N, d).reshape(11, N)
    flat = y_hat.reshape(-1, N)
    cols = []
    for c in range(N):
        z = flat[:, c].contiguous().reshape(-1, 1, 1, 1)
        cols.append(kernels.rate_bits(z, sp[:, c].contiguous())[:, 0])
    return torch.stack(cols, dim=1)


# ------------------------------------------------------------------ 1. picks against float64
@pytest.mark.parametrize("N", [128, 192])
def test_picks_against_float64(device, nets, N):
    net, pack, ys = nets(N)
    p = np_pack(pack)
    moved_total = 0
    for y in ys:
        y_np = y.cpu().numpy()
        for s, rdo, kind, lam in combos(N):
            d = DELTAS[s]
            y_hat, _, _ = kernels.quantise_rdo(y, pack, d, torch.from_numpy(lam).to(device))
            v = y_hat.cpu().numpy()
            t = R.quotient(y_np, d)    # the GPU's own t: quantise_step's ŷ is rint of this quotient
            assert np.array_equal(kernels.quantise_step(y, d)[0].cpu().numpy(), np.rint(t))
            j = R.judge(t, v, p, d, lam)
            share = float(j["near_tie"].mean())
            moved = v != np.rint(t)
            moved_total += int(moved.sum())
            print(f"N={N} {tuple(y.shape)} index {s} lam {rdo} {kind}: moved {moved.mean():.4f}, "
                  f"near ties {int(j['near_tie'].sum())} of {v.size} ({share:.4f}), worst "
                  f"excess/margin {float(np.max(j['excess'] / j['margin'])):.3f}")
            assert j["is_candidate"].all()
            assert (j["excess"] <= j["margin"]).all()
            clear = ~j["near_tie"]
            assert np.array_equal(v[clear], j["argmin"][clear])
            assert share <= R.NEAR_TIE_CAP
    assert moved_total > 0


# ------------------------------------------------------------------ 2. exact properties
@pytest.mark.parametrize("N", [128, 192])
def test_exact_properties(device, nets, N):
    net, pack, ys = nets(N)
    for y in ys:
        for s, rdo, kind, lam in combos(N):
            d = DELTAS[s]
            lam_d = torch.from_numpy(lam).to(device)
            y_hat, y_deq, bits = kernels.quantise_rdo(y, pack, d, lam_d)
            r, r_deq = kernels.quantise_step(y, d)
            assert y_hat.dtype == y_deq.dtype == torch.float32 and bits.dtype == torch.float64
            assert y_hat.shape == y_deq.shape == y.shape and tuple(bits.shape) == (y.shape[0],)
            assert torch.equal(y_deq, kernels.dequantise_step(y_hat, d))      # Δ·ŷ, one product
            assert np.array_equal(y_deq.cpu().numpy(), np.float32(d) * y_hat.cpu().numpy())
            assert torch.equal(y_hat, torch.round(y_hat))
            assert bool((y_hat.abs() <= r.abs()).all())
            assert bool(((y_hat == 0) | (torch.sign(y_hat) == torch.sign(r))).all())
            assert bool(((y_hat == r) | (y_hat == r - torch.sign(r)) | (y_hat == 0)).all())
            # a second call is bitwise equal
            again = kernels.quantise_rdo(y, pack, d, lam_d)
            assert all(torch.equal(a, b) for a, b in zip(again, (y_hat, y_deq, bits)))
            # an image's result does not depend on the batch it travelled in
            for b in range(y.shape[0]):
                alone = kernels.quantise_rdo(y[b:b + 1].contiguous(), pack, d, lam_d)
                assert torch.equal(alone[0], y_hat[b:b + 1]) and torch.equal(alone[1], y_deq[b:b + 1])
                assert torch.equal(alone[2], bits[b:b + 1])
    # element bits never rise, both through the existing rate_bits path (the case that moves most)
    for y in ys:
        d = DELTAS[2]
        lam_d = lam_on(device, 0.25, R.weights(N, "unit"))
        y_hat = kernels.quantise_rdo(y, pack, d, lam_d)[0]
        r = kernels.quantise_step(y, d)[0]
        b_rdo, b_rint = element_bits_gpu(y_hat, pack, N, d), element_bits_gpu(r, pack, N, d)
        moved = (y_hat != r).reshape(-1, N)
        assert bool((b_rdo <= b_rint).all()) and bool((b_rdo[moved] < b_rint[moved]).all())
        assert torch.equal(b_rdo[~moved], b_rint[~moved])


# ------------------------------------------------------------------ 3. bits
def bits_f64(y_hat, pack, d):
    """Σ element bits per image in float64 on the step pack of d: y_hat numpy NHWC."""
    el = R.element_bits(y_hat, pack, d, np.float64)
    return el.reshape(el.shape[0], -1).sum(axis=1)


@pytest.mark.parametrize("N", [128, 192])
def test_bits(device, nets, N):
    net, pack, ys = nets(N)
    p = np_pack(pack)
    for y in ys:
        for rdo, kind in ((0.25, "unit"), (1.0, "ramp"), (16.0, "unit")):
            lam_d = lam_on(device, rdo, R.weights(N, kind))
            sweep = kernels.rate_sweep_rdo(y, pack, DELTAS, lam_d)
            assert sweep.dtype == torch.float64 and tuple(sweep.shape) == (y.shape[0], 32)
            assert torch.equal(kernels.rate_sweep_rdo(y, pack, DELTAS, lam_d), sweep)
            plain = kernels.rate_sweep(y, pack, DELTAS)
            assert bool((sweep <= plain * (1 + 1e-12)).all())
            worst = [0.0, 0.0, 0.0]
            for s, d in enumerate(DELTAS):
                y_hat, _, bits = kernels.quantise_rdo(y, pack, d, lam_d)
                want = rate_bits_of(y_hat, pack, N, d)
                worst[0] = max(worst[0], ((bits - want).abs() / want.abs()).max().item())
                worst[1] = max(worst[1], ((sweep[:, s] - bits).abs() / bits.abs()).max().item())
                f64 = bits_f64(y_hat.cpu().numpy(), p, d)
                worst[2] = max(worst[2], float((np.abs(sweep[:, s].cpu().numpy() - f64) / np.abs(f64)).max()))
            print(f"N={N} {tuple(y.shape)} lam {rdo} {kind}: quantise_rdo vs rate_bits {worst[0]:.3e}, "
                  f"sweep vs quantise_rdo {worst[1]:.3e}, sweep vs float64 {worst[2]:.3e}")
            assert worst[0] <= 1e-12 and worst[1] <= 1e-12 and worst[2] <= R.METRIC_REL
            for s in (0, 8, 31):   # S = 1: a column of the full sweep
                one = kernels.rate_sweep_rdo(y, pack, [DELTAS[s]], lam_d)
                assert tuple(one.shape) == (y.shape[0], 1)
                assert bool(((one[:, 0] - sweep[:, s]).abs() <= 1e-12 * sweep[:, s].abs()).all())
        # the model-level entry: ladder indices, explicit weights
        g = R.weights(N, "ramp")
        lam_d = lam_on(device, 1.0, g)
        assert torch.equal(net.rate_sweep(y, rdo=1.0, rdo_weights=g),
                           kernels.rate_sweep_rdo(y, pack, DELTAS, lam_d))
        assert torch.equal(net.rate_sweep(y, steps=[4, 9], latent=True, rdo=1.0, rdo_weights=g),
                           kernels.rate_sweep_rdo(y, pack, [DELTAS[4], DELTAS[9]], lam_d))
    lam_d = lam_on(device, 1.0, R.weights(N, "unit"))
    for bad in ([], DELTAS + [1.0]):
        with pytest.raises(kernels.Iclr17Error, match="steps"):
            kernels.rate_sweep_rdo(ys[0], pack, bad, lam_d)
    with pytest.raises(kernels.Iclr17Error, match="not finite and positive"):
        kernels.rate_sweep_rdo(ys[0], pack, [1.0, 0.0], lam_d)


# ------------------------------------------------------------------ 4. limits
@pytest.mark.parametrize("N", [128, 192])
def test_limits(device, nets, N):
    net, pack, ys = nets(N)
    p = np_pack(pack)
    zero = torch.zeros(N, device=device)
    for y in ys:
        y_np = y.cpu().numpy()
        for s in R.INDICES:
            d = DELTAS[s]
            t = R.quotient(y_np, d)
            # lam·Δ² ≥ 2^40: the plain quantiser wherever t is not an exact rounding tie
            huge = torch.full((N,), 2.0 ** 41 / (d * d), device=device)
            assert float(huge[0]) * np.float32(d) * np.float32(d) >= 2.0 ** 40
            got = kernels.quantise_rdo(y, pack, d, huge)[0].cpu().numpy()
            off = ~R.exact_tie(t)
            assert np.array_equal(got[off], kernels.quantise_step(y, d)[0].cpu().numpy()[off])
            # lam = 0: the cheapest candidate outside near ties
            got = kernels.quantise_rdo(y, pack, d, zero)[0].cpu().numpy()
            j = R.judge(t, got, p, d, np.zeros(N, np.float32))
            clear = ~j["near_tie"]
            assert np.array_equal(got[clear], R.cheapest(t, p, d, np.float64)[clear])
            assert (j["excess"] <= j["margin"]).all() and j["near_tie"].mean() <= R.NEAR_TIE_CAP
    # exact ties and every branch of the candidate list, with a flat (lam = 0) and a steep cost
    t = torch.tensor([0.4, -0.4, 1.2, -1.2, 2.5, -2.5, 7.3, -7.3, 1.5, 0.5, 40.2, -40.2],
                     device=device).repeat(N).reshape(1, 1, 12, N).contiguous()
    got = kernels.quantise_rdo(t, pack, 1.0, torch.full((N,), 2.0 ** 41, device=device))[0]
    tie = torch.from_numpy(R.exact_tie(t.cpu().numpy())).to(device)
    assert torch.equal(got[~tie], kernels.quantise_step(t, 1.0)[0][~tie])
    # NaN and |r| > 32767 raise as quantise_step does
    y = ys[0]
    lam_d = lam_on(device, 1.0, R.weights(N, "unit"))
    for value, text in ((float("nan"), "a latent is NaN"), (8192.0, "> 32767"),
                        (float("-inf"), "> 32767")):
        bad = y.clone()
        bad[1, 3, 5, N - 1] = value   # the last element
        with pytest.raises(kernels.Iclr17Error, match=text):
            kernels.quantise_rdo(bad, pack, 0.25, lam_d)
    assert float(kernels.quantise_rdo(y.clone().fill_(8191.75), pack, 0.25,
                                      torch.full((N,), 2.0 ** 45, device=device))[0].max()) == 32767.0
    with pytest.raises(kernels.Iclr17Error, match="not finite and positive"):
        kernels.quantise_rdo(y, pack, 0.0, lam_d)
    for bad in (torch.full((N,), -1.0, device=device), torch.full((N,), float("nan"), device=device),
                torch.full((N,), float("inf"), device=device)):
        with pytest.raises(kernels.Iclr17Error, match="lam must be finite and >= 0"):
            kernels.quantise_rdo(y, pack, 1.0, bad)
        with pytest.raises(kernels.Iclr17Error, match="lam must be finite and >= 0"):
            kernels.rate_sweep_rdo(y, pack, [1.0], bad)
    for bad in (torch.ones(N - 1, device=device), torch.ones(N, device=device, dtype=torch.float64),
                torch.ones(N), np.ones(N, np.float32)):
        with pytest.raises(kernels.Iclr17Error, match="lam must be an fp32 tensor"):
            kernels.quantise_rdo(y, pack, 1.0, bad)


# ------------------------------------------------------------------ 5. codec
def to_u8(x_hat):
    """The egress contract on a CPU tensor [..., 3, H, W]: half-to-even of clamp·255."""
    return torch.round(x_hat.clamp(0, 1) * 255).to(torch.uint8)


@pytest.mark.parametrize("precision", ["x6", "h3"])
def test_codec_round_trip(device, nets, precision):
    N = 128
    net, pack, _ = nets(N)
    group = [R.smooth(60 + k, H, W) for k, (H, W) in enumerate(MIXED)]
    fp = codec.fingerprint(net)
    with kernels.precision_scope(precision):
        y = net.latents(R.batch(group).to(device))
        for s, rdo in ((2, 0.25), (8, 1.0), (14, 0.5)):
            blobs = net.compress_images(group, step=s, rdo=rdo)
            enc = net.compress_latents(y, s, rdo=rdo)
            lam_d = (net.synthesis_gains() * rdo).contiguous()
            y_hat, y_deq, bits = kernels.quantise_rdo(y, pack, DELTAS[s], lam_d)
            assert torch.equal(enc["y_hat"], y_hat) and torch.equal(enc["est_bits"], bits)
            plain = net.compress_latents(y, s)
            assert "est_bits" not in plain
            assert bool((y_hat != plain["y_hat"]).any())
            for b, string, im in zip(blobs, enc["strings"], group):
                head, step = codec.parse_blob(b, N=N, fingerprint=fp)
                assert b[:4] == b"I17Q" and step == s and (head.H, head.W) == im.shape[:2]
                assert b[codec.HEADER.size:] == string
            # the unchanged decoder yields exactly ŷ_rdo, and the image of those latents
            dec = net.decompress([b[codec.HEADER.size:] for b in blobs], (4, 6), step=s)
            assert torch.equal(dec["y_hat"], y_hat.permute(0, 3, 1, 2))
            with torch.no_grad():
                want = to_u8(net.Decoder(y_deq.permute(0, 3, 1, 2).contiguous()).clamp(0, 1).cpu())
            for k, (im, got) in enumerate(zip(group, net.decompress_images(blobs))):
                H, W = im.shape[:2]
                assert got.dtype == np.uint8 and got.shape == (H, W, 3)
                assert np.array_equal(got, want[k, :, :H, :W].permute(1, 2, 0).numpy()), (s, k)
            # the estimate falls (or stays) image by image at the same step
            est_plain = rate_bits_of(plain["y_hat"], pack, N, DELTAS[s])
            print(f"{precision} index {s} lam {rdo}: estimated bits {est_plain.sum().item():.1f} -> "
                  f"{bits.sum().item():.1f}, bytes {sum(map(len, net.compress_images(group, step=s)))} "
                  f"-> {sum(map(len, blobs))}")
            assert bool((bits <= est_plain).all()) and bits.sum().item() < est_plain.sum().item()
        # rdo alone: the unit step, an I17Q blob; explicit weights; a blob does not depend on its batch
        alone = net.compress_images(group, rdo=1.0)
        assert alone == net.compress_images(group, step=codec.UNIT_STEP, rdo=1.0)
        assert all(b[:4] == b"I17Q" and codec.parse_blob(b)[1] == codec.UNIT_STEP for b in alone)
        assert net.compress_images(group, rdo=1.0, max_batch=1) == alone
        assert net.compress_images(group[1:2], rdo=1.0) == alone[1:2]
        g = net.synthesis_gains().cpu().numpy()
        assert net.compress_images(group, rdo=1.0, rdo_weights=g) == alone
        assert net.compress_images(group, rdo=1.0, rdo_weights=R.weights(N, "ramp")) != alone
        # mixed with plain, stepped and mapped blobs in one decompress_images call
        stepped = net.compress_images(group, step=13)
        mapped = net.compress_images(group, step=8, step_offsets=[
            np.array([[-3, 2]], np.int8) for _ in group], block=4)
        plain_blobs = net.compress_images(group)
        rd = net.compress_images(group, step=13, rdo=4.0)
        mixed = [plain_blobs[0], rd[1], stepped[2], mapped[3], alone[0], rd[0], mapped[1], stepped[1]]
        assert [b[:4] for b in mixed[:4]] == [b"I17C", b"I17Q", b"I17Q", b"I17M"]
        single = [net.decompress_images([b])[0] for b in mixed]
        for a, b in zip(net.decompress_images(mixed), single):
            assert np.array_equal(a, b)
        for a, b in zip(net.decompress_images(mixed, max_batch=2), single):
            assert np.array_equal(a, b)
        rows = net.evaluate_images(group[:2], step=13, rdo=4.0)
        assert [r["step"] for r in rows] == [13, 13]
        assert [r["bytes"] for r in rows] == [len(b) for b in rd[:2]]
        assert np.array_equal(rows[1]["recon"], net.decompress_images(rd[1:2])[0])
        # without rdo every path writes what it wrote
        assert net.compress_images(group, step=13) == stepped
        with pytest.raises(kernels.Iclr17Error, match="is not built"):
            net.compress_images(group, rdo=1.0, step_offsets=[None] * 4)


@pytest.mark.parametrize("N", [128, 192])
def test_budgets_with_rdo(device, nets, N):
    net, pack, _ = nets(N)
    group = [R.smooth(60 + k, H, W) for k, (H, W) in enumerate(MIXED)]
    sizes = [len(b) for b in net.compress_images(group)]
    budgets = [5 * sizes[0] // 4, sizes[1] // 2, 3 * sizes[2] // 4, sizes[3] // 2]
    base = [codec.parse_blob(b)[1] for b in net.compress_images(group, max_bytes=budgets)]
    overhead = codec.blob_overhead(1)
    y = net.latents(R.batch(group).to(device))
    for rdo in (0.25, 1.0, 16.0):
        stats = {}
        blobs = net.compress_images(group, max_bytes=budgets, rdo=rdo, stats=stats)
        steps = [codec.parse_blob(b)[1] for b in blobs]
        print(f"N={N} lam {rdo}: budgets {budgets}, indices {steps} (without rdo {base}), bytes "
              f"{[len(b) for b in blobs]}, re-encodes {stats['reencodes']}")
        assert all(b[:4] == b"I17Q" and len(b) <= m for b, m in zip(blobs, budgets))
        assert len(stats["reencodes"]) == 4 and all(n >= 0 for n in stats["reencodes"])
        # the first pick is choose_step on the rdo sweep, and a blob is what step= and rdo= write
        est = net.rate_sweep(y, latent=True, rdo=rdo).cpu().numpy()
        for k, (b, s, n) in enumerate(zip(blobs, steps, stats["reencodes"])):
            assert s == codec.choose_step(est[k], budgets[k], overhead) + n
            assert [b] == net.compress_images(group[k:k + 1], step=s, rdo=rdo)
            assert [b] == net.compress_images(group[k:k + 1], max_bytes=budgets[k], rdo=rdo)
        for im, got in zip(group, net.decompress_images(blobs)):
            assert got.shape == im.shape
    assert net.compress_images(group[:2], bpp=2.0, rdo=1.0) == net.compress_images(
        group[:2], max_bytes=[2 * H * W // 8 for H, W in MIXED[:2]], rdo=1.0)


def test_command_line(device, nets, tmp_path, capsys):
    import json

    from PIL import Image
    net, _, _ = nets(128)
    img = R.smooth(61, 64, 96)
    src, out = tmp_path / "in.png", tmp_path / "out.i17c"
    ckpt = tmp_path / "iter_0.pth.tar"
    Image.fromarray(img).save(src)
    torch.save(net.state_dict(), ckpt)
    common = ["--weights", str(ckpt), "--N", "128"]
    for flags, kw in ((["--rdo", "1.0"], {"rdo": 1.0}), (["--step", "13", "--rdo", "4"], {"step": 13, "rdo": 4.0}),
                      (["--max-bytes", "1500", "--rdo", "0.5"], {"max_bytes": 1500, "rdo": 0.5})):
        assert codec.main(["encode", str(src), str(out), *common, *flags]) == 0
        blob = net.compress_images([img], **kw)[0]
        assert out.read_bytes() == blob and blob[:4] == b"I17Q"
    capsys.readouterr()
    assert codec.main(["eval", str(src), *common, "--steps", "4,12", "--rdo", "2"]) == 0
    rows = [json.loads(line) for line in capsys.readouterr().out.strip().splitlines()]
    assert [(r["name"], r["step"], r["rdo"]) for r in rows] == [
        (str(src), 4, 2.0), ("mean", 4, 2.0), (str(src), 12, 2.0), ("mean", 12, 2.0)]
    want = net.evaluate_images([img], step=12, rdo=2.0)[0]
    assert rows[2]["bytes"] == want["bytes"] and rows[2]["psnr_u8"] == want["psnr_u8"]


# ------------------------------------------------------------------ 6. gains
def test_synthesis_gains(device):
    N = 128
    net = make_net(N, device)   # its own: a parameter changes below
    g = net.synthesis_gains()
    assert g.dtype == torch.float32 and tuple(g.shape) == (N,) and g.device.type == "cuda"
    assert net.synthesis_gains() is g
    # the same impulse construction through the oracle in float64
    p = {k: v.double() for k, v in oracle.state_dict_to_torch(synth.trained_like_state_dict(N, 1)).items()}
    probe = torch.zeros(N + 1, N, 8, 8, dtype=torch.float64)
    probe[torch.arange(N), torch.arange(N), 4, 4] = 1.0
    with torch.no_grad():
        out = oracle.synthesis(probe, p)
    assert tuple(out.shape) == (N + 1, 3, 128, 128)
    resp = out[:N] - out[N:]
    # the response fits the output: nothing of it reaches the border
    assert float(resp[:, :, 0].abs().max()) == 0 and float(resp[:, :, :, -1].abs().max()) == 0
    want = (resp ** 2).sum(dim=(1, 2, 3))
    want = want / want.mean()
    rel = ((g.cpu().double() - want).abs() / want).max().item()
    print(f"synthesis gains: min {want.min().item():.3f} max {want.max().item():.3f}, max rel "
          f"error {rel:.3e}")
    assert rel <= R.GRAD_REL
    assert abs(g.double().mean().item() - 1.0) <= 1e-6
    # the same in every precision mode, and invalidated when a parameter changes
    with kernels.precision_scope("h3"):
        assert net.synthesis_gains() is g
    with torch.no_grad():
        net.Decoder.deconv3.weight[5, 1, 2, 2] += 0.25
    fresh = net.synthesis_gains()
    assert fresh is not g and not torch.equal(fresh, g)
    assert abs(fresh.double().mean().item() - 1.0) <= 1e-6
    with torch.no_grad():
        net.bitEstimator.f1.b[0, 0, 0, 0] += 0.0   # any parameter: the cache follows the versions
    assert net.synthesis_gains() is not fresh and torch.equal(net.synthesis_gains(), fresh)
