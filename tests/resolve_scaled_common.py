"""The fetch of ilm_resolve_lighting_scaled restated in numpy float32 (include/illuminant_hip.h defines it): one numpy operation per
rounded operation, in the header's order.  Coverage in double, as the host computes it.  Nothing here asks the library anything."""
import numpy as np

F = np.float32
POINT, LINEAR = 0, 1


def coordinate(n, origin, extent, r0, r1, offset=None):
    """The clamped texel-space coordinate of destination pixels 0 .. n - 1 on one axis:
    u = r0 + (((float)p + 0.5f) - origin) * (r1 - r0) / extent; [+ offset]; fminf(fmaxf(u, r0), r1) -- a NaN becomes r0."""
    with np.errstate(all="ignore"):
        r0, r1 = F(r0), F(r1)
        u = np.arange(n, dtype=np.float32) + F(0.5)
        u = u - F(origin)
        u = u * (r1 - r0)
        u = u / F(extent)
        u = r0 + u
        if offset is not None:
            u = u + F(offset)
        return np.fmin(np.fmax(u, r0), r1)


def taps(u, size, filt):
    """(i0, i1, f) of coordinates u on an axis of `size` texels."""
    if filt == LINEAR:
        s = u - F(0.5)
        fl = np.floor(s)
        f = s - fl
        i = fl.astype(np.int64)
        return np.clip(i, 0, size - 1), np.clip(i + 1, 0, size - 1), f
    i = np.clip(np.floor(u).astype(np.int64), 0, size - 1)
    return i, i, np.zeros(len(u), np.float32)


def _lerp(a, b, t):
    return a + (b - a) * t


def axes(texture_shape, dst_size, quad, region, filt, offset=None):
    """((x0, x1, fx), (y0, y1, fy)) for every column / row of a dst_size = (width, height) target."""
    h, w = texture_shape[:2]
    ox, oy = (None, None) if offset is None else offset
    ux = coordinate(dst_size[0], quad[0], quad[2], region[0], region[2], ox)
    uy = coordinate(dst_size[1], quad[1], quad[3], region[1], region[3], oy)
    return taps(ux, w, filt), taps(uy, h, filt)


def sample(texels, dst_size, quad, region=None, filt=LINEAR, offset=None):
    """The texel every pixel of the target fetches, (height, width, 4) float32 -- covered or not: `coverage` says which are written.
    texels: (h, w, 4) float32, decoded; region None = the whole texture; offset: (x, y) in texels or None."""
    texels = np.ascontiguousarray(texels, np.float32)
    h, w = texels.shape[:2]
    if region is None:
        region = (0.0, 0.0, w, h)
    (x0, x1, fx), (y0, y1, fy) = axes(texels.shape, dst_size, quad, region, filt, offset)
    if filt != LINEAR:
        return texels[y0[:, None], x0[None, :]]
    with np.errstate(all="ignore"):
        fx4, fy4 = fx[None, :, None], fy[:, None, None]
        top = _lerp(texels[y0[:, None], x0[None, :]], texels[y0[:, None], x1[None, :]], fx4)
        bottom = _lerp(texels[y1[:, None], x0[None, :]], texels[y1[:, None], x1[None, :]], fx4)
        return _lerp(top, bottom, fy4)


def point_index(texture_shape, dst_size, quad, region=None, offset=None):
    """The linear index y * width + x of the texel a POINT fetch picks, per pixel of the target."""
    h, w = texture_shape[:2]
    if region is None:
        region = (0.0, 0.0, w, h)
    (x0, _, _), (y0, _, _) = axes(texture_shape, dst_size, quad, region, POINT, offset)
    return y0[:, None] * w + x0[None, :]


def coverage(dst_size, quad, row_begin=0, row_end=None):
    """(height, width) bool: the pixels whose centre lies in [x, x + width) x [y, y + height), rows [row_begin, row_end); in double."""
    width, height = dst_size
    row_end = height if row_end is None else row_end
    x, y, w, h = [float(F(v)) for v in quad]
    cx, cy = np.arange(width, dtype=np.float64) + 0.5, np.arange(height, dtype=np.float64) + 0.5
    rows = np.arange(height)
    in_x = (cx >= x) & (cx < x + w)
    in_y = (cy >= y) & (cy < y + h) & (rows >= row_begin) & (rows < row_end)
    return in_y[:, None] & in_x[None, :]
