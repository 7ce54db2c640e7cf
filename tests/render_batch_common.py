"""Shared by the ilm_engine_render_particles_batch tests: scenes of several systems, the device loop of ilm_render_particles they are held
to, the oracle's loop over one fp32 image, and the picture criterion of tests/test_raster_gpu.py (copied: that file is not edited)."""
import numpy as np

from illuminant_amd import abi, native, scenes

P, RCOL, RD = abi.PLANE_POSITION, abi.PLANE_RENDER_COLOR, abi.PLANE_RENDER_DATA


def random_chunks(seed, cs, n_chunks, width, height, size_hi, dead_fraction=0.3):
    """tests/test_raster_gpu.py::random_chunks: [position+life, velocity, attributes, render colour, render data] per chunk."""
    n = cs * cs
    chunks = []
    for c in range(n_chunks):
        pos = np.zeros((n, 4), np.float32)
        pos[:, 0] = scenes.uniform(seed + 10 * c, (n,), -20.0, width + 20.0)
        pos[:, 1] = scenes.uniform(seed + 10 * c + 1, (n,), -20.0, height + 20.0)
        pos[:, 2] = scenes.uniform(seed + 10 * c + 2, (n,), 0.0, 8.0)
        pos[:, 3] = np.where(scenes.uniform(seed + 10 * c + 3, (n,)) < dead_fraction, 0.0, scenes.uniform(seed + 10 * c + 4, (n,), 0.1, 3.0))
        a = scenes.uniform(seed + 10 * c + 5, (n,), 0.0, 1.0)
        rgb = scenes.uniform(seed + 10 * c + 6, (n, 3), 0.0, 1.0)
        col = np.concatenate([rgb * a[:, None], a[:, None]], axis=1).astype(np.float32)          # premultiplied, some fully transparent
        col[::17, 3] = 0.0
        rd = np.zeros((n, 4), np.float32)
        rd[:, 0] = scenes.uniform(seed + 10 * c + 7, (n,), 0.0, size_hi)
        rd[:, 1] = scenes.uniform(seed + 10 * c + 8, (n,), -7.0, 20.0)                           # rotation, beyond one turn both ways
        chunks.append([pos, np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), col, rd])
    return chunks


def compare_images(got, want, what, max_outliers):
    """tests/test_raster_gpu.py::compare_images: coverage is decided by the same IEEE operations on both sides except sin / cos of the
    rotation (OCML vs libm, a 1e-7 relative difference in the inverse map): a pixel centre within that distance of a rotated edge may fall
    on the other side.  Everything else must agree to 1e-4 * max(1, |want|); at most `max_outliers` pixels may differ by a whole fragment."""
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max(axis=-1)
    tol = 1e-4 * np.maximum(1.0, np.abs(want).max(axis=-1))
    bad = err > tol
    assert int(bad.sum()) <= max_outliers, "%s: %d pixels differ (largest %.3g)" % (what, int(bad.sum()), float(err.max()))


class Item:
    """One item of a batch on both sides: the device system, and the planes / bitmap the oracle reads."""

    def __init__(self, system, chunks, params, quad_counts=None, bitmap=None):
        self.system, self.chunks, self.params, self.quad_counts, self.bitmap = system, chunks, params, quad_counts, bitmap

    def native(self):
        return (self.system, self.params, self.quad_counts)


def make_system(engine, chunks, bitmap=None):
    sysm = native.System(engine)
    for c, planes in enumerate(chunks):
        sysm.add_chunk()
        sysm.upload(c, P, planes[0]); sysm.upload(c, RCOL, planes[3]); sysm.upload(c, RD, planes[4])
    if bitmap is not None:
        sysm.set_bitmap(bitmap)
    return sysm


def device_loop(items, target):
    """ilm_render_particles item after item: what the batch is defined against.  Returns the summed stats."""
    total = [0, 0, 0]
    for it in items:
        st = native.render_particles(it.system, it.params, target, quad_counts=it.quad_counts, want_stats=True)
        total = [a + b for a, b in zip(total, st)]
    return tuple(total)


def oracle_loop(oracle, items, image):
    """The CPU reference of every picture: the oracle's render applied item after item on ONE fp32 image.  Returns (live, shaded) summed."""
    live = shaded = 0
    h, w = image.shape[:2]
    for it in items:
        if not it.chunks:
            continue
        image, (l, s) = oracle.render_particles(it.chunks, it.params, w, h, quad_counts=it.quad_counts, image=image, bitmap=it.bitmap)
        live += l; shaded += s
    return image, (live, shaded)


def filled(width, height, rgba):
    image = np.zeros((height, width, 4), np.float32)
    image[:] = rgba
    return image
