"""Hand-made tables and latents for the entropy coder's edge tests (csrc/rans.hip against
oracle/rans_ref.py): frequency tables at the ends of the 16-bit range, latents that drive a stream
to the ends of what a symbol can cost, and the shapes at which a stream has 1, 42, 63, 64, 65, 128
and 336 symbols. Nothing here is a model's table: the coder takes any valid cumulative row.

A table row holds 2K + 3 cumulative frequencies over the 2K + 2 symbols of a channel: the values
−K..K as symbols 0..2K, then the escape. A symbol of frequency 1 always costs a renormalisation
word; an escape always costs its payload word as well. A stream of nsym escapes at escape
frequency 1 therefore has 128 + 2·nsym words, the capacity of its scratch slot exactly.
"""
import functools
import zlib

import numpy as np

from oracle import rans_ref

PROB_SCALE = 1 << 16
LANES = 64

KS = (1, 4, 32)
BASE_FAMILIES = ("floor", "edges", "escape", "uniform")
FAMILIES = BASE_FAMILIES + ("mixed",)
SEQUENCES = ("all_escape", "all_peak", "all_floor", "alternating", "random")

# (B, h, w, N, P): nsym = (N/P)·h·w symbols per stream
SHAPES = (
    (2, 1, 1, 16, 16),    # 1: one symbol, 63 idle lanes
    (1, 3, 7, 16, 8),     # 42: a partial block spanning two channels
    (1, 7, 9, 16, 16),    # 63: just under one block, one channel
    (1, 3, 7, 24, 8),     # 63: a block spanning three channels
    (1, 8, 8, 16, 16),    # 64: exactly one block
    (1, 5, 13, 16, 16),   # 65: one symbol in the last block
    (1, 8, 8, 32, 16),    # 128: two full blocks
    (2, 3, 7, 16, 1),     # 336: a ragged last block of 16
)
RAGGED_TILES = (1, 9, 9, 16, 2)   # at t = 8: tiles of 64, 8, 8 and 1 positions


def nsym(shape):
    B, h, w, N, P = shape
    return N // P * h * w


def shape_id(shape):
    return "x".join(map(str, shape))


def row(freq):
    """2K + 2 frequencies → the cumulative row of 2K + 3 entries."""
    f = np.asarray(freq, dtype=np.int64)
    assert f.ndim == 1 and f.size >= 4 and f.size % 2 == 0
    assert (f >= 1).all() and int(f.sum()) == PROB_SCALE
    return np.concatenate([[0], np.cumsum(f)]).astype(np.int64)


def frequencies(family, K):
    """The 2K + 2 frequencies of one row of a base family."""
    NS = 2 * K + 2
    f = np.ones(NS, dtype=np.int64)
    if family == "floor":        # value 0 takes all but one slot per other symbol
        f[K] = PROB_SCALE - (NS - 1)
    elif family == "edges":      # −K and +K share the rest
        rest = PROB_SCALE - (NS - 2)
        f[0], f[2 * K] = rest // 2, rest - rest // 2
    elif family == "escape":     # f << 16 just below 2^32
        f[NS - 1] = PROB_SCALE - (NS - 1)
    elif family == "uniform":
        q, r = divmod(PROB_SCALE, NS)
        f[:] = q
        f[:r] += 1
    else:
        raise ValueError(family)
    return f


def mixed_row(c, K, s=0):
    """Row c of ``mixed`` moved on by s: family (c + s) mod 4, its frequencies rotated by
    c + s // 4 symbols. s = 0 is ``mixed`` itself: family c mod 4 rotated by c."""
    return row(np.roll(frequencies(BASE_FAMILIES[(c + s) % 4], K), c + s // 4))


def table(family, N, K):
    """int64 [N, 2K + 3]. A base family repeats its row; ``mixed`` gives channel c the family
    c mod 4 rotated by c, so neighbouring channels never share a row."""
    if family == "mixed":
        return np.stack([mixed_row(c, K) for c in range(N)])
    return np.tile(row(frequencies(family, K)), (N, 1))


def stacked(S, N, K):
    """int64 [S, N, 2K + 3] for the mapped coder: set s is ``mixed`` moved on by s (``mixed_row``),
    so set 0 is ``mixed`` and a wrong slot codes with another row. Neighbouring sets differ in
    every channel. Any two of 32 sets differ in at least half the channels at K > 1 (a rotated
    ``floor`` row can be a rotated ``escape`` row); at K = 1 a row has four symbols and only 13
    distinct rows exist."""
    return np.stack([np.stack([mixed_row(c, K, s) for c in range(N)]) for s in range(S)])


def slot_map(S, B, h, w, block, seed=0):
    """uint8 [B, mh, mw] with every set 0..S−1 where the map has room, else as many as fit."""
    mh, mw = -(-h // block), -(-w // block)
    n = B * mh * mw
    rng = np.random.default_rng(_seed("slots", S, B, h, w, block, seed))
    m = np.concatenate([np.arange(S)[:min(S, n)], rng.integers(0, S, max(0, n - S))])
    return rng.permutation(m).astype(np.uint8).reshape(B, mh, mw)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _rows(cum, shape, slots, block):
    """The row of every element, [B, h, w, N, 2K + 3]."""
    B, h, w, N, P = shape
    cum = np.asarray(cum)
    if cum.ndim == 2:
        return np.broadcast_to(cum[None, None, None], (B, h, w) + cum.shape)
    pos = np.asarray(slots)[:, (np.arange(h) // block)[:, None], (np.arange(w) // block)[None, :]]
    return cum[pos]            # [B, h, w] indexes the sets → [B, h, w, N, 2K + 3]


def stream_position(shape):
    """Each element's index in its stream of the plain layout, [h, w, N]: symbols run in
    (channel, row, column) order over the group's channels."""
    B, h, w, N, P = shape
    cl = np.arange(N) % (N // P)
    return (cl[None, None, :] * h + np.arange(h)[:, None, None]) * w + np.arange(w)[None, :, None]


def latent(name, shape, K, cum, slots=None, block=1, seed=0):
    """The sequence ``name`` as an NHWC float32 latent [B, h, w, N] for the tables ``cum``
    ([N, 2K + 3], or [S, N, 2K + 3] with the slot map ``slots`` of block edge ``block``).

    all_escape   values from {K+1, −K−1, 1000, 32767, −32767}: payload and symbol every time
    all_peak     each element its row's most frequent symbol (K + 1 where that is the escape)
    all_floor    each element an in-range value of frequency 1 (where a row has none, as in
                 ``uniform``, its least frequent in-range value)
    alternating  all_floor and all_peak by the parity of lane + block of the plain layout
    random       uniform over −K−2 .. K+2
    """
    B, h, w, N, P = shape
    rng = np.random.default_rng(_seed(name, shape, K, seed))
    full = (B, h, w, N)
    if name == "all_escape":
        y = rng.choice(np.array([K + 1, -K - 1, 1000, 32767, -32767]), size=full)
    elif name == "random":
        y = rng.integers(-K - 2, K + 3, size=full)
    else:
        freq = np.diff(_rows(cum, shape, slots, block), axis=-1)      # [B, h, w, N, 2K + 2]
        top = freq.argmax(axis=-1)
        peak = np.where(top == 2 * K + 1, K + 1, top - K)
        low = freq[..., :2 * K + 1].argmin(axis=-1) - K
        if name == "all_peak":
            y = peak
        elif name == "all_floor":
            y = low
        elif name == "alternating":
            i = stream_position(shape)
            y = np.where(((i % LANES + i // LANES) % 2 == 0)[None], low, peak)
        else:
            raise ValueError(name)
    return np.ascontiguousarray(y, dtype=np.float32).reshape(full)


@functools.lru_cache(maxsize=None)
def plain_case(family, sequence, K, shape):
    """(ŷ, tables int64, the oracle's words and offsets) of one case; computed once per process
    and shared: callers must not write to the arrays."""
    B, h, w, N, P = shape
    cum = table(family, N, K)
    y = latent(sequence, shape, K, cum)
    words, offsets = rans_ref.encode(y, cum, K, P)
    for a in (y, cum, words, offsets):
        a.setflags(write=False)
    return y, cum, words, offsets


def stream_words(words, offsets):
    return [words[offsets[s]:offsets[s + 1]].tolist() for s in range(len(offsets) - 1)]


def _tile_words(y, cum, K, P, t, b, r, c, g):
    """encode_stream of group g of tile (r, c) of image b: its (channel, row, column) sequence."""
    cpg = y.shape[3] // P
    tile = y[b, r * t:(r + 1) * t, c * t:(c + 1) * t]      # ragged at the edges
    chans = np.arange(g * cpg, (g + 1) * cpg)
    values = tile[:, :, chans].transpose(2, 0, 1).reshape(-1).astype(np.int64)
    rows = np.repeat(chans, tile.shape[0] * tile.shape[1])
    return rans_ref.encode_stream(values.tolist(), rows.tolist(), cum, K)


def tile_streams(y, cum, K, P, t):
    """The oracle's words of every tile stream, in (image, tile row, tile column, group) order."""
    B, h, w, N = y.shape
    return [_tile_words(y, cum, K, P, t, b, r, c, g) for b in range(B) for r in range(-(-h // t))
            for c in range(-(-w // t)) for g in range(P)]


def tile_stream(y, cum, K, P, t, s):
    """Stream s of ``tile_streams`` alone, its place worked out from the index."""
    B, h, w, N = y.shape
    th, tw = -(-h // t), -(-w // t)
    q, g = divmod(s, P)
    q, c = divmod(q, tw)
    b, r = divmod(q, th)
    return _tile_words(y, cum, K, P, t, b, r, c, g)
