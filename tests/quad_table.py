"""numpy restatement of the luma quad table (csrc/device_math.hpp: pack_quad, KfDev::quads), shared by
tests/test_quad_table_cpu.py and tests/test_gpu_quad_table.py."""
import numpy as np


def pack_quad(tl, tr, bl, br):
    """pack_quad: the differences in integers, each converted to fp16.  Returns (..., 4) float16 {tl, dtop, dleft, dmix}."""
    tl, tr, bl, br = (np.asarray(v, np.int32) for v in (tl, tr, bl, br))
    dtop = tr - tl
    return np.stack([tl, dtop, bl - tl, (br - bl) - dtop], axis=-1).astype(np.float16)


def table(luma):
    """The table of one (h, w) u8 luma image: (h + 1, w + 1, 4) float16, entry [j + 1][i + 1] = the footprint of base texel (i, j)
    with clamp addressing, i in [-1, w - 1], j in [-1, h - 1]."""
    h, w = luma.shape
    i0 = np.clip(np.arange(-1, w), 0, w - 1)
    i1 = np.clip(np.arange(0, w + 1), 0, w - 1)
    j0 = np.clip(np.arange(-1, h), 0, h - 1)
    j1 = np.clip(np.arange(0, h + 1), 0, h - 1)
    return pack_quad(luma[np.ix_(j0, i0)], luma[np.ix_(j0, i1)], luma[np.ix_(j1, i0)], luma[np.ix_(j1, i1)])


def unpack_bytes(entry):
    """unpack_quad_bytes: tl, tr, bl, br by float32 adds of the converted entry."""
    e = np.asarray(entry, np.float16).astype(np.float32)
    tl, dtop, dleft, dmix = e[..., 0], e[..., 1], e[..., 2], e[..., 3]
    bl = tl + dleft
    return tl, tl + dtop, bl, bl + (dmix + dtop)
