"""Scenes that pin the particle rasteriser's machinery (raster.hip): known run lengths per tile, sprites that belong to one quadrant,
tile tables of chosen sizes, pair totals at the cap -- and numpy references for what the oracle does not report.

Every sprite is axis-aligned (rotation exactly 0.0), square-cornered and untextured: sin / cos are exactly 0 and 1 and no pow runs, so
device and oracle execute the same IEEE operations (-ffp-contract=off on both sides) and a FLOAT4 frame whose tiles all take the direct
path can be compared bit for bit.  No GPU is needed by anything in this module.

A scene builder returns (chunks, quad_counts, params, width, height); what it claims about its tiles comes from a separate *_claims
function that looks only at how the scene was laid out, never at tile_runs."""
import functools

import numpy as np

from illuminant_amd import abi, scenes

TILE = 16
SEGMENT = 2048            # kRasterSegment
BATCH = 256               # the LDS batch of raster_tiles_kernel
GLOBAL_COLOR = (0.9, 0.8, 1.0, 0.7)
CLEAR = (0.05, 0.1, 0.15, 0.2)
FAINT = 0.15              # as test_crowded_tiles_are_shaded_in_segments: thousands of layers still change the pixel

A_W, A_H, A_TILE = 64, 48, (2, 1)      # scene (a): the crowded tile is neither the first nor on an image border
RUN_LENGTHS = (1, 255, 256, 257, 2047, 2048, 2049, 4096, 4097)


def raster_params(blend=abi.BLEND_ALPHA, dithered=False):
    """Positions are pixels, RenderData.x is the half extent in pixels."""
    return scenes.rasterize_params(global_color=GLOBAL_COLOR[:3] + (1.0,) if dithered else GLOBAL_COLOR, rounded=False, blend=blend,
                                   dithered_opacity=dithered)


# ---- packing ---------------------------------------------------------------------------------------------------------------------

def colors(seed, n, faint=FAINT):
    """premultiplied RenderColor, alpha in [0.2, 1) x faint"""
    a = scenes.uniform(seed, (n,), 0.2, 1.0)
    rgb = scenes.uniform(seed + 1, (n, 3), 0.0, 1.0)
    return (np.concatenate([rgb * a[:, None], a[:, None]], axis=1) * np.float32(faint)).astype(np.float32)


def pack(x, y, half, color, cs, width, height, life=None, z=None, n_chunks=None):
    """Sprites in slot order -> chunks of cs * cs slots in random_chunks' plane layout (position+life, -, -, RenderColor, RenderData)
    and the quad counts that end the last chunk after the last sprite.  The slots behind the quad count hold a live, opaque, magenta
    sprite in the middle of the frame: whoever reads past quad_counts paints it."""
    n, slots = len(x), cs * cs
    count = max(1, -(-n // slots)) if n_chunks is None else n_chunks
    pos = np.zeros((count * slots, 4), np.float32)
    pos[:, 0], pos[:, 1], pos[:, 3] = width * 0.5, height * 0.5, 1.0
    col = np.zeros((count * slots, 4), np.float32)
    col[:] = (1.0, 0.0, 1.0, 1.0)
    rd = np.zeros((count * slots, 4), np.float32)
    rd[:, 0] = 3.0
    pos[:n, 0], pos[:n, 1] = x, y
    pos[:n, 2] = 0.0 if z is None else z
    pos[:n, 3] = 1.0 if life is None else life
    col[:n] = color
    rd[:n, 0] = half
    chunks, quads = [], []
    for c in range(count):
        s = slice(c * slots, (c + 1) * slots)
        planes = [pos[s].copy(), np.zeros((slots, 4), np.float32), np.zeros((slots, 4), np.float32), col[s].copy(), rd[s].copy()]
        for a in planes:
            a.flags.writeable = False              # shared between tests
        chunks.append(planes)
        quads.append(int(min(slots, max(0, n - c * slots))))
    return chunks, quads


def exchange(chunks, first, second):
    """A copy of `chunks` with the sprites of the global slots `first` and `second` (equal-length index arrays) exchanged."""
    slots = chunks[0][0].shape[0]
    out = [[a.copy() for a in planes] for planes in chunks]
    first, second = np.asarray(first), np.asarray(second)
    for k in (0, 3, 4):
        flat = np.concatenate([planes[k] for planes in out], axis=0)
        flat[np.concatenate([first, second])] = flat[np.concatenate([second, first])]
        for c, planes in enumerate(out):
            planes[k] = np.ascontiguousarray(flat[c * slots:(c + 1) * slots])
    return out


# ---- geometry helpers ------------------------------------------------------------------------------------------------------------

def inside_tile(seed, n, tx, lo=1.0, hi=6.0, ty=None):
    """n sprites whose bounding box -- with the rasteriser's pixel of slack on every side -- stays inside tile column tx (and tile
    row ty, where given): they make pairs with that tile alone.  Returns (x, y_or_None, half)."""
    e = scenes.uniform(seed, (n,), lo, hi)
    span = np.float32(12.5) - 2.0 * e                       # centre - half >= tile + 1.75, centre + half <= tile + 14.25
    x = (np.float32(TILE * tx) + 1.75 + e + scenes.uniform(seed + 1, (n,)) * span).astype(np.float32)
    y = None
    if ty is not None:
        y = (np.float32(TILE * ty) + 1.75 + e + scenes.uniform(seed + 2, (n,)) * span).astype(np.float32)
    return x, y, e


def covers(tx, ty):
    """Four sprites of half extent 3.75 on the quadrant centres of a tile: they lie strictly inside it and between them hold every
    one of its 256 pixel centres.  Their bounding boxes (a pixel of slack) reach the neighbouring tiles: each side neighbour gets two
    pairs, each corner neighbour one."""
    x = np.array([4.0, 12.0, 4.0, 12.0], np.float32) + TILE * tx
    y = np.array([4.0, 4.0, 12.0, 12.0], np.float32) + TILE * ty
    return x, y, np.full(4, 3.75, np.float32)


def cover_claims(tx, ty, tiles_x, tiles_y):
    out = {}
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if (dx or dy) and 0 <= tx + dx < tiles_x and 0 <= ty + dy < tiles_y:
                out[(tx + dx, ty + dy)] = 1 if (dx and dy) else 2
    return out


def crowd(seed, n, tx, ty, one_row=False):
    """n sprites that make pairs with tile (tx, ty): n - 4 random ones inside it and the four covers spread through the slot order
    (n < 5: random ones only).  one_row: the frame is one tile row high, the clip to the target keeps y inside."""
    m = n - 4 if n >= 5 else n
    x, y, e = inside_tile(seed, m, tx, ty=None if one_row else ty)
    if one_row:
        y = scenes.uniform(seed + 2, (m,), 0.5, 12.5)
    if n < 5:
        return x, y, e
    cx, cy, ce = covers(tx, ty)
    at = np.array([(k * n) // 5 for k in range(1, 5)])
    keep = np.ones(n, bool)
    keep[at] = False
    ox, oy, oe = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.float32)
    ox[keep], oy[keep], oe[keep] = x, y, e
    ox[at], oy[at], oe[at] = cx, cy, ce
    return ox, oy, oe


# ---- (a) one crowded tile ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def one_tile_scene(n, blend=abi.BLEND_ALPHA, dithered=False, width=A_W, height=A_H, tile=A_TILE):
    """n sprites on one tile, chunk size 64 (4097 crosses a chunk boundary).  Dithered fragments are opaque, so that variant keeps
    the full alphas (a faint fragment never passes the dither) and an alpha of exactly 1 on the four covers and in GlobalColor: the
    covers pass every dither level, so every pixel of the tile is drawn."""
    x, y, e = crowd(1000 + n, n, tile[0], tile[1])
    col = colors(2000 + n, n, faint=1.0 if dithered else FAINT)
    if dithered and n >= 5:
        col[[(k * n) // 5 for k in range(1, 5)], 3] = 1.0
    col[-1] = np.asarray([0.02, 0.6, 0.1, 0.8], np.float32) * np.float32(1.0 if dithered else FAINT)       # the last layer is a visible one
    chunks, quads = pack(x, y, e, col, 64, width, height)
    return chunks, quads, raster_params(blend, dithered), width, height


def one_tile_claims(n, width=A_W, height=A_H, tile=A_TILE):
    tiles_x, tiles_y = (width + 15) // 16, (height + 15) // 16
    claims = {(tx, ty): 0 for ty in range(tiles_y) for tx in range(tiles_x)}
    if n >= 5:
        claims.update(cover_claims(tile[0], tile[1], tiles_x, tiles_y))
    claims[tile] = n
    return claims


def reordered(n, chunks):
    """The exchange that a scene of n sprites on one tile must be able to see: two segments' worth for n >= 4096, last against first
    for 2049."""
    if n >= 2 * SEGMENT:
        return exchange(chunks, np.arange(0, SEGMENT), np.arange(SEGMENT, 2 * SEGMENT))
    return exchange(chunks, [0], [n - 1])


# ---- (b) neighbouring tiles cut at different sprites ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def straddle_scene(blend=abi.BLEND_ALPHA):
    """2048 sprites across the edge between tiles (2, 1) and (3, 1); slot 1000 lies in (2, 1) only, the last slot in (3, 1) only: both
    tiles hold 2049 sprites, (2, 1) is cut after a straddling sprite (its second segment is the last straddler), (3, 1) after all of
    them (its second segment is the lone last sprite)."""
    n = SEGMENT
    e = scenes.uniform(3000, (n,), 3.0, 5.0)
    sx = (47.0 + scenes.uniform(3001, (n,), 0.0, 2.0)).astype(np.float32)         # edge at x = 48: centre - half < 46, centre + half > 50
    sy = (np.float32(17.75) + e + scenes.uniform(3002, (n,)) * (np.float32(12.5) - 2.0 * e)).astype(np.float32)
    lx, ly, le = inside_tile(3003, 1, 2, ty=1, lo=4.0, hi=5.0)
    rx, ry, re = inside_tile(3004, 1, 3, ty=1, lo=4.0, hi=5.0)
    x = np.concatenate([sx[:1000], lx, sx[1000:], rx])
    y = np.concatenate([sy[:1000], ly, sy[1000:], ry])
    h = np.concatenate([e[:1000], le, e[1000:], re])
    chunks, quads = pack(x, y, h, colors(3010, n + 2), 64, A_W, A_H)
    return chunks, quads, raster_params(blend), A_W, A_H


def straddle_claims():
    claims = {(tx, ty): 0 for ty in range(3) for tx in range(4)}
    claims[(2, 1)] = claims[(3, 1)] = SEGMENT + 1
    return claims


# ---- (c) quadrant lists --------------------------------------------------------------------------------------------------------------

QUADRANT_ARRANGEMENTS = ("all_in_3", "round_robin", "one_wave_one_list", "lone_257th", "border_tile")


def quadrant_of_slot(arrangement, n):
    slot = np.arange(n)
    if arrangement == "all_in_3":
        return np.full(n, 3)
    if arrangement == "round_robin":
        return slot % 4
    if arrangement == "one_wave_one_list":
        return (slot // 64) % 4                      # loader wave w of a batch feeds list w alone
    if arrangement == "lone_257th":
        return np.where(slot == BATCH, 0, 1 + slot % 3)
    raise ValueError(arrangement)


@functools.lru_cache(maxsize=None)
def quadrant_scene(arrangement):
    """Sprites of half extent <= 1.5 centred within a pixel of a quadrant's centre: with the pixel of slack each passes the box test of
    its own quadrant only (the next centre is 8 away: 7 - 2.5 > 3.5).  border_tile: the last tile of a 37 x 21 target, quadrant 0
    crowded and itself cut by both borders, quadrants 1-3 outside the image; every tenth sprite sits on one of those quadrants' centres
    (live, no pixel)."""
    if arrangement == "border_tile":
        n, w, h, tile = 300, 37, 21, (2, 1)
        quadrant = np.where(np.arange(n) % 10 == 9, 1 + (np.arange(n) // 10) % 3, 0)
    else:
        n = BATCH + 1 if arrangement == "lone_257th" else 300
        w, h, tile = A_W, A_H, A_TILE
        quadrant = quadrant_of_slot(arrangement, n)
    seed = 4000 + 10 * QUADRANT_ARRANGEMENTS.index(arrangement)
    e = scenes.uniform(seed, (n,), 0.6, 1.5)
    x = (np.float32(TILE * tile[0] + 4) + 8.0 * (quadrant & 1) + scenes.uniform(seed + 1, (n,), -1.0, 1.0)).astype(np.float32)
    y = (np.float32(TILE * tile[1] + 4) + 8.0 * (quadrant >> 1) + scenes.uniform(seed + 2, (n,), -1.0, 1.0)).astype(np.float32)
    chunks, quads = pack(x, y, e, colors(seed + 3, n, faint=0.5), 64, w, h)
    return chunks, quads, raster_params(), w, h


def quadrant_claims(arrangement):
    if arrangement == "border_tile":
        claims = {(tx, ty): 0 for ty in range(2) for tx in range(3)}
        claims[(2, 1)] = 300 - 30
        return claims
    claims = {(tx, ty): 0 for ty in range(3) for tx in range(4)}
    claims[A_TILE] = BATCH + 1 if arrangement == "lone_257th" else 300
    return claims


# ---- (e) tile tables: one tile row, two crowded tiles far apart -------------------------------------------------------------------------

STRIPS = ((1022, 16), (1023, 13), (1024, 16), (9216, 13))        # tiles + 1 = 1023, 1024, 1025 (per = 1, 1, 2) and 9217 (per = 10)
STRIP_RUNS = (SEGMENT + 1, 2 * SEGMENT + 1)                      # a third of the way along, and on the last tile


def strip_layout(tiles):
    """(crowded tiles, tiles the background may use, background count)"""
    crowded = (tiles // 3, tiles - 1)
    shut = {t + d for t in crowded for d in (-1, 0, 1)}
    free = np.array([t for t in range(tiles) if t not in shut])
    return crowded, free, max(3000, tiles)


@functools.lru_cache(maxsize=None)
def strip_background(tiles):
    """(tile, x, half extent) of the background sprites: each inside one tile, none on the crowded tiles or next to them"""
    _, free, n_bg = strip_layout(tiles)
    tile_of = free[(scenes.uniform(5000 + tiles, (n_bg,)) * len(free)).astype(np.int64)]
    e = scenes.uniform(5001 + tiles, (n_bg,), 1.0, 4.0)
    x = (tile_of * TILE + 1.75 + e + scenes.uniform(5002 + tiles, (n_bg,)) * (np.float32(12.5) - 2.0 * e)).astype(np.float32)
    return tile_of, x, e


@functools.lru_cache(maxsize=None)
def strip_scene(tiles, height):
    """A frame one tile row high: the background, 2049 sprites on the tile a third of the way along and 4097 on the last tile, shuffled
    into each other in slot order."""
    crowded, _, n_bg = strip_layout(tiles)
    _, bx, e = strip_background(tiles)
    xs, ys, es = [bx], [scenes.uniform(5003 + tiles, (n_bg,), 0.0, float(height))], [e]
    for k, (t, n) in enumerate(zip(crowded, STRIP_RUNS)):
        x, y, h = crowd(5010 + tiles + k, n, t, 0, one_row=True)
        xs.append(x); ys.append(y); es.append(h)
    x, y, h = np.concatenate(xs), np.concatenate(ys), np.concatenate(es)
    order = np.argsort(scenes.uniform(5020 + tiles, (len(x),)), kind="stable")
    chunks, quads = pack(x[order], y[order], h[order], colors(5030 + tiles, len(x)), 64, tiles * TILE, height)
    return chunks, quads, raster_params(), tiles * TILE, height


def strip_claims(tiles):
    crowded, _, _ = strip_layout(tiles)
    runs = np.bincount(strip_background(tiles)[0], minlength=tiles).astype(np.int64)
    for t, n in zip(crowded, STRIP_RUNS):
        runs[t] = n
        for d in (-1, 1):
            if 0 <= t + d < tiles:
                runs[t + d] += 2                    # two covers reach each side neighbour
    return runs.reshape(1, tiles)


TINY_TARGETS = ((1, 1), (7, 5), (16, 16), (17, 16), (16, 17))
TINY_SPRITES = {(1, 1): 1, (7, 5): 4, (16, 16): 2, (17, 16): 3, (16, 17): 4}


@functools.lru_cache(maxsize=None)
def tiny_scene(width, height):
    """One to four sprites on a target of a tile or two: the first is larger than the whole target, the third sits on the right
    border (the second tile column of 17 x 16), the fourth on the bottom border (the second tile row of 16 x 17)."""
    n = TINY_SPRITES[(width, height)]
    x = np.array([0.5 * width, 0.4 * width, width - 0.75, 0.25], np.float32)[:n]
    y = np.array([0.5 * height, 0.6 * height, 0.3, height - 0.5], np.float32)[:n]
    e = np.array([40.0, 0.75, 1.5, 2.25], np.float32)[:n]
    chunks, quads = pack(x, y, e, colors(6000 + width * 31 + height, n, faint=0.6), 16, width, height)
    return chunks, quads, raster_params(), width, height


# ---- (f) the pair cap ------------------------------------------------------------------------------------------------------------------

CAP_W = CAP_H = 4096                  # 65 536 tiles
CAP_PAIRS = 1 << 28


@functools.lru_cache(maxsize=None)
def cap_scene(kind):
    """Sprites that cover the whole 4096 x 4096 frame make 65 536 pairs each.  "one_over": 4096 of them and one sprite inside a single
    tile, 2^28 + 1 pairs.  "wrap": 65 536 of them fill a 256 x 256-slot chunk and an empty second chunk follows, so the exclusive sum at
    the last slot is exactly 2^32 -- 0 in 32 bits unless the scan saturates.  Both are refused; nothing is drawn."""
    n = 4096 if kind == "one_over" else 65536
    x = np.full(n, 2048.0, np.float32) + scenes.uniform(7000, (n,), -8.0, 8.0)
    y = np.full(n, 2048.0, np.float32) + scenes.uniform(7001, (n,), -8.0, 8.0)
    e = np.full(n, 3000.0, np.float32)
    if kind == "one_over":
        x, y, e = np.append(x, np.float32(1000.0)), np.append(y, np.float32(2008.0)), np.append(e, np.float32(2.0))
    chunks, quads = pack(x, y, e, colors(7002, len(x)), 256, CAP_W, CAP_H, n_chunks=1 if kind == "one_over" else 2)
    return chunks, quads, raster_params(), CAP_W, CAP_H


# ---- (g) non-finite and degenerate slots -----------------------------------------------------------------------------------------------

def degenerate_slots():
    """(what, x, y, z, life, half extent, alpha multiplier, counts as live)"""
    nan, inf = float("nan"), float("inf")
    f = np.float32
    return [
        ("life NaN", 10.0, 9.0, 0.0, nan, 3.0, 1.0, True),               # `life <= 0` is false for a NaN: drawn, as in the shader
        ("life -0", 12.0, 9.0, 0.0, -0.0, 3.0, 1.0, False),
        ("life +0", 14.0, 9.0, 0.0, 0.0, 3.0, 1.0, False),
        ("life denormal", 16.0, 9.0, 0.0, float(f(1e-40)), 3.0, 1.0, True),
        ("life smallest denormal", 18.0, 9.0, 0.0, float(np.frombuffer(np.uint32(1).tobytes(), np.float32)[0]), 3.0, 1.0, True),
        ("life negative", 20.0, 9.0, 0.0, -1.0, 3.0, 1.0, False),
        ("life -inf", 22.0, 9.0, 0.0, -inf, 3.0, 1.0, False),
        ("life +inf", 24.0, 9.0, 0.0, inf, 3.0, 1.0, True),
        ("size 0", 10.0, 20.0, 0.0, 1.0, 0.0, 1.0, False),
        ("size -0", 11.0, 20.0, 0.0, 1.0, -0.0, 1.0, False),
        ("size negative", 13.0, 20.0, 0.0, 1.0, -2.5, 1.0, True),         # a mirrored quad: det > 0, the unit test still decides
        ("size 1e18", 24.0, 16.0, 0.0, 1.0, 1e18, 0.2, True),             # det = 1e36 is finite: covers every pixel
        ("size 1e30", 24.0, 16.0, 0.0, 1.0, 1e30, 1.0, False),            # det overflows
        ("size inf", 24.0, 16.0, 0.0, 1.0, inf, 1.0, False),              # 0 * inf = NaN
        ("size NaN", 24.0, 16.0, 0.0, 1.0, nan, 1.0, False),
        ("size denormal", 24.0, 16.0, 0.0, 1.0, float(f(1e-30)), 1.0, False),   # det underflows to 0
        ("x NaN", nan, 16.0, 0.0, 1.0, 3.0, 1.0, False),
        ("y NaN", 24.0, nan, 0.0, 1.0, 3.0, 1.0, False),
        ("z NaN", 24.0, 16.0, nan, 1.0, 3.0, 1.0, False),
        ("x +inf", inf, 16.0, 0.0, 1.0, 3.0, 1.0, False),
        ("x -inf", -inf, 16.0, 0.0, 1.0, 3.0, 1.0, False),
        ("y +inf", 24.0, inf, 0.0, 1.0, 3.0, 1.0, False),
        ("y -inf", 24.0, -inf, 0.0, 1.0, 3.0, 1.0, False),
        ("z +inf", 24.0, 16.0, inf, 1.0, 3.0, 1.0, False),                # inf * 0 = NaN in the display position
        ("z -inf", 24.0, 16.0, -inf, 1.0, 3.0, 1.0, False),
        ("x 1e30", 1e30, 16.0, 0.0, 1.0, 3.0, 1.0, True),                 # finite and far away: live, no pair
        ("x -1e30", -1e30, 16.0, 0.0, 1.0, 3.0, 1.0, True),
        ("y 1e30", 24.0, 1e30, 0.0, 1.0, 3.0, 1.0, True),
        ("y -1e30", 24.0, -1e30, 0.0, 1.0, 3.0, 1.0, True),
        ("x 3e38 size 3e9", 3e38, 16.0, 0.0, 1.0, 3e9, 1.0, True),
        ("just off the left", -5.0, 16.0, 0.0, 1.0, 3.0, 1.0, True),
        ("just off the bottom", 24.0, 37.0, 0.0, 1.0, 3.0, 1.0, True),
        ("half on the right border", 47.5, 12.0, 0.0, 1.0, 3.0, 1.0, True),
        ("alpha 0", 30.0, 10.0, 0.0, 1.0, 4.0, 0.0, True),                # live, never shaded
        ("alpha -0", 31.0, 10.0, 0.0, 1.0, 4.0, -0.0, True),
        ("alpha negative", 32.0, 10.0, 0.0, 1.0, 4.0, -0.5, True),
        ("alpha 1.5", 34.0, 12.0, 0.0, 1.0, 4.0, 1.5 / 0.7, True),        # x GlobalColor.w = 0.7: a fragment alpha above 1, keep < 0
        ("alpha 1", 36.0, 22.0, 0.0, 1.0, 4.0, 1.0 / 0.7, True),
    ]


DEGENERATE_W, DEGENERATE_H, ORDINARY = 48, 32, 120


@functools.lru_cache(maxsize=None)
def degenerate_scene():
    """The hand-placed slots of degenerate_slots(), one after every third ordinary sprite."""
    special = degenerate_slots()
    n = ORDINARY + len(special)
    at = 1 + 3 * np.arange(len(special))
    keep = np.ones(n, bool)
    keep[at] = False
    x, y, z, life, e = (np.zeros(n, np.float32) for _ in range(5))
    col = colors(8003, n, faint=0.5)
    x[keep] = scenes.uniform(8000, (ORDINARY,), -4.0, DEGENERATE_W + 4.0)
    y[keep] = scenes.uniform(8001, (ORDINARY,), -4.0, DEGENERATE_H + 4.0)
    e[keep] = scenes.uniform(8002, (ORDINARY,), 0.5, 7.0)
    life[keep] = 1.0
    base = np.asarray([0.3, 0.6, 0.2, 1.0], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, (_, sx, sy, sz, sl, se, sa, _) in zip(at, special):
            x[i], y[i], z[i], life[i], e[i] = sx, sy, sz, sl, se
            col[i] = base * np.float32(sa)
    chunks, quads = pack(x, y, e, col, 16, DEGENERATE_W, DEGENERATE_H, life=life, z=z)
    return chunks, quads, raster_params(), DEGENERATE_W, DEGENERATE_H


def degenerate_live_claim():
    return ORDINARY + sum(1 for s in degenerate_slots() if s[-1])


# ---- (h) frames for the scratch-reuse sequence ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scattered_scene(width, height, n, seed):
    x = scenes.uniform(seed, (n,), -4.0, width + 4.0)
    y = scenes.uniform(seed + 1, (n,), -4.0, height + 4.0)
    e = scenes.uniform(seed + 2, (n,), 0.5, 9.0)
    chunks, quads = pack(x, y, e, colors(seed + 3, n, faint=0.5), 64, width, height)
    return chunks, quads, raster_params(), width, height


# ---- references ------------------------------------------------------------------------------------------------------------------------

def tile_runs(chunks, quad_counts, params, width, height):
    """(runs[tiles_y, tiles_x], pairs): how many sprites make a pair with each tile, and the total -- the setup kernel's bounding-box
    arithmetic for unrotated sprites in float32, in the expression order of raster_sprite and of the clip in
    orc_render_particles_textured (oracle/ilm_oracle_output.c).  sin = 0 and cos = 1 exactly."""
    f = np.float32
    p = params
    tiles_x, tiles_y = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
    diff = np.zeros((tiles_y + 1, tiles_x + 1), np.int64)
    pairs = 0
    with np.errstate(all="ignore"):
        for planes, quads in zip(chunks, quad_counts if quad_counts is not None else [None] * len(chunks)):
            count = planes[0].shape[0] if quads is None else min(int(quads), planes[0].shape[0])
            pos, rd = planes[0][:count], planes[4][:count]
            assert np.all(rd[:, 1] == 0.0), "tile_runs restates unrotated sprites only"
            px, py, pz, life = pos[:, 0], pos[:, 1], pos[:, 2], pos[:, 3]
            alive = ~(life <= f(0.0))
            sx = (rd[:, 0] * f(p.SystemSize[0])) * f(p.SizeFactorAndPosition.x)
            sy = (rd[:, 0] * f(p.SystemSize[1])) * f(p.SizeFactorAndPosition.y)
            zf = np.fmax(f(0.0), f(1.0) + (pz * f(p.ZConfiguration.x)))             # fmaxf: a NaN loses
            sx, sy = sx * zf, sy * zf
            s, c = f(0.0), f(1.0)
            display_x = (px * f(p.Scale.x)) + f(p.SizeFactorAndPosition.z)
            display_y = ((py - (pz * f(p.ZToY))) * f(p.Scale.y)) + f(p.SizeFactorAndPosition.w)
            cx = (display_x - f(p.ViewportPosition[0])) * f(p.ViewportScale[0])
            cy = (display_y - f(p.ViewportPosition[1])) * f(p.ViewportScale[1])
            kx, ky = f(p.Scale.x) * f(p.ViewportScale[0]), f(p.Scale.y) * f(p.ViewportScale[1])
            a00, a01 = (c * sx) * kx, -(s * sy) * kx
            a10, a11 = (s * sx) * ky, (c * sy) * ky
            det = (a00 * a11) - (a01 * a10)
            alive &= (np.abs(det) > f(0.0)) & np.isfinite(det) & np.isfinite(cx) & np.isfinite(cy)
            ex, ey = np.abs(a00) + np.abs(a01), np.abs(a10) + np.abs(a11)
            fx0, fx1 = np.floor(cx - ex - f(0.5)) - f(1.0), np.ceil(cx + ex - f(0.5)) + f(1.0)
            fy0, fy1 = np.floor(cy - ey - f(0.5)) - f(1.0), np.ceil(cy + ey - f(0.5)) + f(1.0)
            fx0, fy0 = np.where(fx0 < 0, f(0.0), fx0), np.where(fy0 < 0, f(0.0), fy0)
            fx1, fy1 = np.where(fx1 > f(width - 1), f(width - 1), fx1), np.where(fy1 > f(height - 1), f(height - 1), fy1)
            alive &= (fx0 <= fx1) & (fy0 <= fy1)
            tx0, tx1 = fx0[alive].astype(np.int64) // TILE, fx1[alive].astype(np.int64) // TILE
            ty0, ty1 = fy0[alive].astype(np.int64) // TILE, fy1[alive].astype(np.int64) // TILE
            pairs += int(((tx1 - tx0 + 1) * (ty1 - ty0 + 1)).sum())
            np.add.at(diff, (ty0, tx0), 1)
            np.add.at(diff, (ty0, tx1 + 1), -1)
            np.add.at(diff, (ty1 + 1, tx0), -1)
            np.add.at(diff, (ty1 + 1, tx1 + 1), 1)
    runs = diff.cumsum(axis=0).cumsum(axis=1)[:tiles_y, :tiles_x]
    assert int(runs.sum()) == pairs
    return runs, pairs


def is_direct(runs):
    """every tile's run fits one segment: each is blended straight into the target, in the oracle's order of operations"""
    return int(runs.max()) <= SEGMENT


def to_target(image, fmt):
    """float32 (h, w, 4) -> the target's own texels: float16 by round-to-nearest-even, unorm8 as rint(sat(x) * 255) in float32"""
    image = np.asarray(image, np.float32)
    if fmt == abi.LIGHTMAP_FLOAT4:
        return image.copy()
    if fmt == abi.LIGHTMAP_HALF4:
        with np.errstate(over="ignore"):
            return image.astype(np.float16)          # IEEE round-to-nearest-even
    sat = np.minimum(np.maximum(image, np.float32(0.0)), np.float32(1.0))
    return np.rint(sat * np.float32(255.0)).astype(np.uint8)


def from_target(texels, fmt):
    """the float32 values the rasteriser's load_target reads from such texels"""
    if fmt == abi.LIGHTMAP_FLOAT4:
        return np.asarray(texels, np.float32).copy()
    if fmt == abi.LIGHTMAP_HALF4:
        return np.asarray(texels).view(np.float16).astype(np.float32)
    return np.asarray(texels, np.uint8).astype(np.float32) / np.float32(255.0)


def initial_content(width, height, fmt, seed=9000):
    """A gradient plus noise in the target's format: below 1 for RGBA8, up to about 4 for HALF4."""
    top = 4.0 if fmt == abi.LIGHTMAP_HALF4 else 0.999
    jj, ii = np.mgrid[0:height, 0:width]
    ramp = (ii / max(1, width - 1) * 0.6 + jj / max(1, height - 1) * 0.25)[..., None] * np.asarray([1.0, 0.8, 0.6, 0.9])
    noise = scenes.uniform(seed, (height, width, 4), 0.0, 0.15)
    return to_target((np.minimum(ramp + noise, 1.0) * top).astype(np.float32), fmt)


def half_steps(got, want):
    """distance in representable float16 values between two float16 arrays of finite numbers"""
    def key(a):
        bits = np.asarray(a, np.float16).view(np.uint16).astype(np.int32)
        return np.where(bits & 0x8000, -(bits & 0x7FFF), bits)
    return np.abs(key(got) - key(want))


def unorm8_codes(want):
    """(code, near_tie): rint(sat(want) * 255) and where want * 255 lies within 1e-3 of a tie between two codes"""
    sat = np.minimum(np.maximum(np.asarray(want, np.float32), np.float32(0.0)), np.float32(1.0))
    scaled = sat * np.float32(255.0)
    frac = scaled.astype(np.float64) - np.floor(scaled.astype(np.float64))
    return np.rint(scaled).astype(np.int32), np.abs(frac - 0.5) <= 1e-3


# ---- the oracle's picture of a scene, computed once ----------------------------------------------------------------------------------------

_REFERENCES = {}


def reference(oracle, key, scene, initial=None):
    """(image, (live, shaded), (runs, pairs)) of a scene, from the oracle and tile_runs, computed once per key and shared read-only.
    initial: the float32 content the target starts from (default: CLEAR everywhere)."""
    if key not in _REFERENCES:
        chunks, quads, params, w, h = scene[:5]
        image = np.zeros((h, w, 4), np.float32)
        image[:] = np.asarray(CLEAR, np.float32) if initial is None else initial
        image, stats = oracle.render_particles(chunks, params, w, h, quad_counts=quads, image=image)
        image.flags.writeable = False
        _REFERENCES[key] = (image, stats, tile_runs(chunks, quads, params, w, h))
    return _REFERENCES[key]


def same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32))
