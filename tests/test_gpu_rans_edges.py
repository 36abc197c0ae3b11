"""The entropy coder (csrc/rans.hip) where the model's tables never take it: hand-made tables at
the ends of the frequency range, streams that fill their scratch slot to the last word, tables at
the LDS limit, and more than 1024 streams. Every comparison is exact: words and offsets against
oracle/rans_ref.py, decoded latents bit for bit.

The cases are those of tests/rans_cases.py (tests/test_rans_cases_cpu.py shows the stated lengths
for the oracle alone). The slot tests call the entry points on scratch the test owns: guards of
4096 words on either side of the slots and every unwritten word hold a pattern, so a write outside
a stream's slot is a failed assertion inside the test's own allocation.

Measured on one MI355X: the module's 167 tests in 8.5 s, the slowest case 0.3 s; the oracle's
per-symbol Python is most of it (every case has fewer than 2100 symbols, the two many-stream cases
check 2080 one-symbol streams and 32 sampled tile streams).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import rans_cases as C
import stepmap_refs as R
from iclr_17_compression_amd import _lib, codec, kernels, synth
from iclr_17_compression_amd.model import ImageCompressor
from oracle import rans_ref

pytestmark = pytest.mark.gpu

G = 4096                 # guard words (elements) on either side of a buffer the test owns
PATTERN = 0x5A5A         # every scratch word before the call
SENTINEL = -12345.5      # every output element before a decode: no latent is a half
T = 8                    # the tile edge; log2 = 3
ALL_SHAPES = C.SHAPES + (C.RAGGED_TILES,)
PAST = "ran past its words"

shapes = pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
shapes_and_ragged = pytest.mark.parametrize("shape", ALL_SHAPES, ids=C.shape_id)
ks = pytest.mark.parametrize("K", C.KS)


# ------------------------------------------------------------------ helpers
def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream_of(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def on(device, a, dtype=None):
    """A numpy array (possibly read-only) as a device tensor."""
    return torch.tensor(np.asarray(a, dtype=dtype), device=device)


def tables_on(device, cum):
    return on(device, cum, np.int32)


def u16(t):
    return t.cpu().numpy().view(np.uint16)


def words_on(device, words):
    return on(device, np.asarray(words, dtype=np.uint16).view(np.int16))


def join(streams):
    """Per-stream word lists → (uint16 words, int64 offsets)."""
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    return np.array([w for s in streams for w in s], dtype=np.uint16), offsets


def assert_coded(words, offsets, ref_w, ref_o, what):
    assert np.array_equal(offsets.cpu().numpy(), ref_o), what
    assert np.array_equal(u16(words), ref_w), what


def one_tile(shape):
    return shape[1] <= T and shape[2] <= T


@functools.lru_cache(maxsize=None)
def tiled_case(family, sequence, K, shape):
    """The oracle's words of every tile stream at t = 8; one tile: the plain streams."""
    y, cum, words, offsets = C.plain_case(family, sequence, K, shape)
    if one_tile(shape):
        return C.stream_words(words, offsets)
    return C.tile_streams(y, cum, K, shape[4], T)


@functools.lru_cache(maxsize=None)
def map_case(sequence, K, shape, S, block):
    """(ŷ, stacked tables, slot map, the oracle's words of every stream) of a mapped case."""
    B, h, w, N, P = shape
    st = C.stacked(S, N, K)
    slots = C.slot_map(S, B, h, w, block)
    y = C.latent(sequence, shape, K, st, slots, block)
    rows = st.reshape(S * N, 2 * K + 3)
    streams = []
    for b in range(B):
        for grp in range(P):
            values, chans = R.stream_symbols(y[b], slots[b], block, N, P, grp)
            streams.append(rans_ref.encode_stream(values, chans, rows, K))
    return y, st, slots, streams


def guarded_encode(device, ns, cap, launch):
    """Runs ``launch(scratch pointer, scratch words, lengths, status)`` on G + ns·cap + G pattern
    words, the pointer at word G → (the whole buffer as uint16, lengths [ns], the word after the
    lengths, status)."""
    buf = torch.full((G + ns * cap + G,), PATTERN, dtype=torch.int16, device=device)
    lengths = torch.full((ns + 1,), -1, dtype=torch.int32, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    launch(ptr(buf[G:]), ns * cap, ptr(lengths), ptr(status))
    torch.cuda.synchronize()
    ln = lengths.cpu().numpy().view(np.uint32)
    return u16(buf), ln[:ns].astype(np.int64), int(ln[ns]), int(status.item())


def assert_slots(got, ns, cap, streams, what, full=False):
    """Every stream inside its slot: guards and leading words untouched, the trailing words the
    oracle's; ``full``: every slot used to its first word."""
    buf, lengths, after, status = got
    assert status == 0 and after == 0xFFFFFFFF, what
    assert len(streams) == ns and (lengths <= cap).all(), (what, lengths.max(), cap)
    assert (buf[:G] == PATTERN).all() and (buf[G + ns * cap:] == PATTERN).all(), what
    assert lengths.tolist() == [len(s) for s in streams], what
    for s in range(ns):
        slot = buf[G + s * cap:G + (s + 1) * cap]
        n = int(lengths[s])
        assert (slot[:cap - n] == PATTERN).all(), (what, s)
        assert slot[cap - n:].tolist() == streams[s], (what, s)
    if full:
        assert (lengths == cap).all(), (what, lengths.tolist(), cap)


def guarded_decode(device, shape4, launch):
    """Runs ``launch(output pointer, output elements, status)`` on G + numel + G sentinel floats,
    the pointer at element G → the decoded latent, after checking both guards and the status."""
    numel = int(np.prod(shape4))
    buf = torch.full((G + numel + G,), SENTINEL, dtype=torch.float32, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    launch(ptr(buf[G:]), numel, ptr(status))
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    out = buf.cpu().numpy()
    assert (out[:G] == np.float32(SENTINEL)).all() and (out[G + numel:] == np.float32(SENTINEL)).all()
    return out[G:G + numel].reshape(shape4)


# ------------------------------------------------------------------ 1. words, three layouts
@shapes
@ks
def test_plain_words_equal_the_oracle(device, K, shape):
    B, h, w, N, P = shape
    for family in C.FAMILIES:
        for sequence in C.SEQUENCES:
            y, cum, ref_w, ref_o = C.plain_case(family, sequence, K, shape)
            yd, cd = on(device, y), tables_on(device, cum)
            words, offsets = kernels.rans_encode(yd, cd, K, P)
            assert_coded(words, offsets, ref_w, ref_o, (family, sequence))
            assert torch.equal(kernels.rans_decode(words, offsets, cd, B, h, w, N, K, P), yd), \
                (family, sequence)


@shapes_and_ragged
@ks
def test_tile_words_equal_the_oracle(device, K, shape):
    """A latent of one tile: the plain coder's words. 5×13 is tiles of 5×8 and 5×5, 7×9 of 7×8 and
    7×1, 9×9 of 8×8, 8×1, 1×8 and 1×1 positions; each stream is encode_stream of its sequence."""
    B, h, w, N, P = shape
    for family in C.FAMILIES:
        for sequence in C.SEQUENCES:
            y, cum, _, _ = C.plain_case(family, sequence, K, shape)
            ref_w, ref_o = join(tiled_case(family, sequence, K, shape))
            assert ref_o.size - 1 == B * -(-h // T) * -(-w // T) * P
            yd, cd = on(device, y), tables_on(device, cum)
            for waves in (1, 4):
                words, offsets = kernels.rans_encode_tiled(yd, cd, T, K, P, waves=waves)
                assert_coded(words, offsets, ref_w, ref_o, (family, sequence, waves))
                back = kernels.rans_decode_tiled(words, offsets, cd, B, h, w, N, T, K, P, waves=waves)
                assert torch.equal(back, yd), (family, sequence, waves)
            if one_tile(shape):   # the layouts describe the same streams
                pw, po = kernels.rans_encode(yd, cd, K, P)
                assert torch.equal(pw, words) and torch.equal(po, offsets), (family, sequence)
                assert torch.equal(kernels.rans_decode(words, offsets, cd, B, h, w, N, K, P), yd)


@shapes
@ks
def test_mapped_words_equal_the_oracle(device, K, shape):
    B, h, w, N, P = shape
    mixed = tables_on(device, C.table("mixed", N, K))
    for sequence in C.SEQUENCES:
        for S in (1, 3, 32):
            for block in (1, 4):
                y, st, slots, streams = map_case(sequence, K, shape, S, block)
                ref_w, ref_o = join(streams)
                yd, sd = on(device, y), tables_on(device, st)
                what = (sequence, S, block)
                for window in (True, False):
                    words, offsets = kernels.rans_encode_map(yd, sd, slots, block, K, P, window=window)
                    assert_coded(words, offsets, ref_w, ref_o, what + (window,))
                    back = kernels.rans_decode_map(words, offsets, sd, slots, block, B, h, w, N, K, P,
                                                   window=window)
                    assert torch.equal(back, yd), what + (window,)
                if S == 1:   # one set, `mixed`: the plain coder's streams
                    pw, po = kernels.rans_encode(yd, mixed, K, P)
                    assert torch.equal(pw, words) and torch.equal(po, offsets), what
        # S identical sets under a map that uses them all: the plain coder's words again
        y = on(device, C.latent(sequence, shape, K, C.table("mixed", N, K)))
        pw, po = kernels.rans_encode(y, mixed, K, P)
        same = torch.stack([mixed] * 3)
        for block in (1, 4):
            slots = C.slot_map(3, B, h, w, block, seed=1)
            for window in (True, False):
                mw, mo = kernels.rans_encode_map(y, same, slots, block, K, P, window=window)
                assert torch.equal(mw, pw) and torch.equal(mo, po), (sequence, block, window)
                back = kernels.rans_decode_map(pw, po, same, slots, block, B, h, w, N, K, P,
                                               window=window)
                assert torch.equal(back, y), (sequence, block, window)


# ------------------------------------------------------------------ 2. the slot is never left
@shapes
@ks
def test_plain_streams_stay_in_their_slots(device, K, shape):
    B, h, w, N, P = shape
    ns, cap = B * P, 128 + 2 * C.nsym(shape)   # the test's own count, the library's asked below
    for family in C.FAMILIES:
        for sequence in C.SEQUENCES:
            y, cum, ref_w, ref_o = C.plain_case(family, sequence, K, shape)
            yd, cd = on(device, y), tables_on(device, cum)
            st = stream_of(yd)
            got = guarded_encode(device, ns, cap, lambda scratch, nwords, lengths, status: _lib.call(
                "iclr17_rans_encode", ptr(yd), B, h, w, N, P, ptr(cd), K, scratch, nwords, lengths,
                status, st))
            assert_slots(got, ns, cap, C.stream_words(ref_w, ref_o), (family, sequence),
                         full=sequence == "all_escape" and family in ("floor", "edges"))
            wd, od = words_on(device, ref_w), on(device, ref_o)
            back = guarded_decode(device, y.shape, lambda out, numel, status: _lib.call(
                "iclr17_rans_decode", ptr(wd), ptr(od), B, h, w, N, P, ptr(cd), K, out, status, st))
            assert np.array_equal(back, y), (family, sequence)
    assert _lib.query("iclr17_rans_capacity", h, w, N, P) == cap


@shapes_and_ragged
@ks
def test_tile_streams_stay_in_their_slots(device, K, shape):
    B, h, w, N, P = shape
    th, tw = -(-h // T), -(-w // T)
    ns, cap = B * th * tw * P, 128 + 2 * (N // P) * T * T
    assert _lib.query("iclr17_rans_tiled_streams", h, w, P, 3) * B == ns
    for family in C.FAMILIES:
        for sequence in C.SEQUENCES:
            y, cum, _, _ = C.plain_case(family, sequence, K, shape)
            streams = tiled_case(family, sequence, K, shape)
            yd, cd = on(device, y), tables_on(device, cum)
            st = stream_of(yd)
            tight = sequence == "all_escape" and family in ("floor", "edges")
            for waves in (0, 1, 4):
                got = guarded_encode(device, ns, cap, lambda scratch, nwords, lengths, status: _lib.call(
                    "iclr17_rans_encode_tiled", ptr(yd), B, h, w, N, P, 3, ptr(cd), K, waves, scratch,
                    nwords, lengths, status, st))
                # a slot holds a full 8×8 tile: exactly full where the tile is one
                assert_slots(got, ns, cap, streams, (family, sequence, waves),
                             full=tight and (h, w) == (T, T))
                if tight:   # every tile stream is as long as its own symbols allow
                    want = [128 + 2 * (N // P) * min(T, h - r * T) * min(T, w - c * T)
                            for _ in range(B) for r in range(th) for c in range(tw) for _ in range(P)]
                    assert got[1].tolist() == want and max(want) <= cap
                    assert shape != C.RAGGED_TILES or want[0] == cap
            ref_w, ref_o = join(streams)
            wd, od = words_on(device, ref_w), on(device, ref_o)
            for waves in (0, 1, 4):
                back = guarded_decode(device, y.shape, lambda out, numel, status: _lib.call(
                    "iclr17_rans_decode_tiled", ptr(wd), int(ref_w.size), ptr(od), B, h, w, N, P, 3,
                    0, 0, th, tw, ptr(cd), K, waves, out, numel, status, st))
                assert np.array_equal(back, y), (family, sequence, waves)
    assert _lib.query("iclr17_rans_tiled_capacity", N, P, 3) == cap


@shapes
@ks
def test_mapped_streams_stay_in_their_slots(device, K, shape):
    B, h, w, N, P = shape
    ns, cap = B * P, 128 + 2 * C.nsym(shape)

    def run(y, st, slots, block, streams, what, full=False):
        S = st.shape[0]
        yd, sd, sl = on(device, y), tables_on(device, st), on(device, slots)
        lg = kernels.MAP_BLOCKS.index(block)
        stm = stream_of(yd)
        ref_w, ref_o = join(streams)
        wd, od = words_on(device, ref_w), on(device, ref_o)
        for window in (1, 0):
            got = guarded_encode(device, ns, cap, lambda scratch, nwords, lengths, status: _lib.call(
                "iclr17_rans_encode_map", ptr(yd), B, h, w, N, P, ptr(sd), S, K, ptr(sl), lg, window,
                scratch, nwords, lengths, status, stm))
            assert_slots(got, ns, cap, streams, what + (window,), full=full)
            back = guarded_decode(device, y.shape, lambda out, numel, status: _lib.call(
                "iclr17_rans_decode_map", ptr(wd), ptr(od), B, h, w, N, P, ptr(sd), S, K, ptr(sl), lg,
                window, out, status, stm))
            assert np.array_equal(back, y), what + (window,)

    for sequence in C.SEQUENCES:
        for S in (1, 3, 32):
            for block in (1, 4):
                y, st, slots, streams = map_case(sequence, K, shape, S, block)
                run(y, st, slots, block, streams, (sequence, S, block))
    # escapes only at escape frequency 1 in every set: each slot exactly full
    for family in ("floor", "edges"):
        y, cum, ref_w, ref_o = C.plain_case(family, "all_escape", K, shape)
        for S, block in ((3, 1), (32, 4)):
            run(y, np.stack([cum] * S), C.slot_map(S, B, h, w, block), block,
                C.stream_words(ref_w, ref_o), (family, S, block), full=True)


# ------------------------------------------------------------------ 3. at the LDS limit
@pytest.mark.parametrize("N,K", [(192, 41), (128, 62)])
def test_tables_at_the_lds_limit(device, N, K):
    """N·(2K + 3)·4 bytes of tables: 65 280 and 65 024 of the 65 536 a workgroup may stage; one
    more symbol pair does not fit and is refused, not truncated."""
    assert N * (2 * K + 3) * 4 <= 65536 < N * (2 * K + 5) * 4
    shape = (1, 2, 3, N, 1)
    B, h, w, _, P = shape
    cum = C.table("mixed", N, K)
    cd = tables_on(device, cum)
    for sequence in ("random", "all_escape"):
        y = C.latent(sequence, shape, K, cum)
        ref_w, ref_o = rans_ref.encode(y, cum, K, P)
        yd = on(device, y)
        words, offsets = kernels.rans_encode(yd, cd, K, P)
        assert_coded(words, offsets, ref_w, ref_o, sequence)
        assert torch.equal(kernels.rans_decode(words, offsets, cd, B, h, w, N, K, P), yd)
        for waves in (1, 4):
            tw_, to_ = kernels.rans_encode_tiled(yd, cd, T, K, P, waves=waves)
            assert torch.equal(tw_, words) and torch.equal(to_, offsets), (sequence, waves)
            back = kernels.rans_decode_tiled(words, offsets, cd, B, h, w, N, T, K, P, waves=waves)
            assert torch.equal(back, yd), (sequence, waves)
    big = tables_on(device, C.table("mixed", N, K + 1))
    for call in (lambda: kernels.rans_encode(yd, big, K + 1, P),
                 lambda: kernels.rans_decode(words, offsets, big, B, h, w, N, K + 1, P),
                 lambda: kernels.rans_encode_tiled(yd, big, T, K + 1, P),
                 lambda: kernels.rans_decode_tiled(words, offsets, big, B, h, w, N, T, K + 1, P)):
        with pytest.raises(kernels.Iclr17Error, match="exceed LDS"):
            call()


# ------------------------------------------------------------------ 4. many streams
@pytest.mark.parametrize("n", [0, 1, 2, 1023, 1024, 1025, 1500, 2048, 2049, 100003])
def test_offsets_scan_equals_cumsum(device, n):
    """One workgroup of 1024 threads, ⌈n/1024⌉ lengths each: the thresholds around 1024 and 2048,
    a ragged last thread, and sums past 2^32 (lengths only: no buffer of that size exists)."""
    rng = np.random.default_rng(1000 + n)
    for lo, hi in ((128, 801), (1 << 31, 1 << 32)):
        lengths = rng.integers(lo, hi, size=max(n, 1), dtype=np.uint32)
        want = np.concatenate([[0], np.cumsum(lengths[:n].astype(np.int64))])
        ld = on(device, lengths.view(np.int32))
        out = torch.full((n + 1 + 64,), -7, dtype=torch.int64, device=device)
        _lib.call("iclr17_rans_offsets", ptr(ld), n, ptr(out), stream_of(out))
        got = out.cpu().numpy()
        assert np.array_equal(got[:n + 1], want), (n, lo)
        assert (got[n + 1:] == -7).all(), (n, lo)
        assert want[-1] >= n * lo   # the second round's sums are past 2^31 from the first length on


def test_2080_streams_of_one_symbol(device):
    shape, K = (130, 1, 1, 16, 16), 4
    B, h, w, N, P = shape
    cum = C.table("mixed", N, K)
    y = C.latent("random", shape, K, cum)
    assert (np.abs(y) > K).any() and B * P == 2080
    ref_w, ref_o = rans_ref.encode(y, cum, K, P)
    yd, cd = on(device, y), tables_on(device, cum)
    words, offsets = kernels.rans_encode(yd, cd, K, P)
    assert_coded(words, offsets, ref_w, ref_o, "plain")
    assert torch.equal(kernels.rans_decode(words, offsets, cd, B, h, w, N, K, P), yd)


def test_1320_tile_streams_at_every_workgroup_shape(device):
    """8 images of 33×257 positions at t = 8: 5×33 tiles each, the last row of tiles one position
    high, the last column one wide. The words do not depend on the waves per workgroup, chosen
    (None) or given; 32 streams, the ragged ones among them, are the oracle's."""
    shape, K = (8, 33, 257, 16, 1), 4
    B, h, w, N, P = shape
    th, tw = 5, 33
    ns = B * th * tw * P
    assert ns == 1320
    cum = C.table("mixed", N, K)
    y = C.latent("random", shape, K, cum)
    yd, cd = on(device, y), tables_on(device, cum)
    coded = {waves: kernels.rans_encode_tiled(yd, cd, T, K, P, waves=waves) for waves in (None, 1, 4)}
    words, offsets = coded[None]
    for waves in (1, 4):
        assert torch.equal(coded[waves][0], words) and torch.equal(coded[waves][1], offsets), waves
    wn, off = u16(words), offsets.cpu().numpy()
    assert off.shape == (ns + 1,) and off[0] == 0 and off[-1] == wn.size
    rng = np.random.default_rng(1320)
    picked = {0, ns - 1, tw - 1, (th - 1) * tw, th * tw - 1, th * tw, 1024, 1023}
    picked |= set(rng.choice(ns, 32 - len(picked), replace=False).tolist())
    for s in sorted(picked)[:32]:
        assert wn[off[s]:off[s + 1]].tolist() == C.tile_stream(y, cum, K, P, T, s), s
    for waves in (None, 1, 4):
        back = kernels.rans_decode_tiled(words, offsets, cd, B, h, w, N, T, K, P, waves=waves)
        assert torch.equal(back, yd), waves


# ------------------------------------------------------------------ 5. the model's tables, every step
@pytest.mark.parametrize("N", [128, 192])
def test_ladder_tables_are_valid_and_code_word_for_word(device, N):
    net = ImageCompressor(out_channel_N=N)
    net.load_state_dict({k: torch.from_numpy(v)
                         for k, v in synth.trained_like_state_dict(N, 1).items()})
    net = net.to(device).eval()
    for K in C.KS:
        for e in range(codec.STEPS):
            t = net.bitEstimator.entropy_tables(K, step=e)
            assert t.dtype == torch.int32 and tuple(t.shape) == (N, 2 * K + 3), (K, e)
            cum = t.cpu().numpy()
            assert (cum[:, 0] == 0).all() and (cum[:, -1] == 65536).all(), (K, e)
            assert (np.diff(cum, axis=1) >= 1).all(), (K, e)
    K, shape = 4, (1, 3, 7, N, 8)
    B, h, w, _, P = shape
    y = C.latent("random", shape, K, None)
    yd = on(device, y)
    for e in (0, codec.STEPS - 1):
        cd = net.bitEstimator.entropy_tables(K, step=e)
        ref_w, ref_o = rans_ref.encode(y, cd.cpu().numpy().astype(np.int64), K, P)
        words, offsets = kernels.rans_encode(yd, cd, K, P)
        assert_coded(words, offsets, ref_w, ref_o, e)
        assert torch.equal(kernels.rans_decode(words, offsets, cd, B, h, w, N, K, P), yd), e


# ------------------------------------------------------------------ 6. a stream shorter than its states
def test_a_stream_of_127_words_is_reported_by_every_decoder(device):
    """A good stream with nothing but its length changed: 127 words, one fewer than the 64 states
    take, so each decoder reports it before it reads a payload word."""
    shape, K = (1, 3, 7, 16, 1), 4
    B, h, w, N, P = shape
    y, cum, ref_w, ref_o = C.plain_case("mixed", "random", K, shape)
    assert ref_o.tolist() == [0, ref_w.size] and ref_w.size > 128
    cd, words = tables_on(device, cum), words_on(device, ref_w)
    good, short = on(device, ref_o), on(device, np.array([0, 127], dtype=np.int64))
    same = torch.stack([cd])
    slots = np.zeros((B, h, w), dtype=np.uint8)
    yd = on(device, y)
    assert torch.equal(kernels.rans_decode(words, good, cd, B, h, w, N, K, P), yd)
    assert torch.equal(kernels.rans_decode_tiled(words, good, cd, B, h, w, N, T, K, P), yd)
    assert torch.equal(kernels.rans_decode_map(words, good, same, slots, 1, B, h, w, N, K, P), yd)
    with pytest.raises(kernels.Iclr17Error, match=PAST):
        kernels.rans_decode(words, short, cd, B, h, w, N, K, P)
    for waves in (1, 4):
        with pytest.raises(kernels.Iclr17Error, match=PAST):
            kernels.rans_decode_tiled(words, short, cd, B, h, w, N, T, K, P, waves=waves)
    for window in (True, False):
        with pytest.raises(kernels.Iclr17Error, match=PAST):
            kernels.rans_decode_map(words, short, same, slots, 1, B, h, w, N, K, P, window=window)
