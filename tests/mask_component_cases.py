"""Masks shared by the component-filter tests (CPU and GPU): random fields and the structures that break
labelling kernels. Every builder returns a u8 [H, W] array of {0, 1}."""
import numpy as np

DENSITIES = (0.05, 0.3, 0.41, 0.9)  # 0.41: near the 8-connected percolation threshold


def random_mask(H, W, density, seed=0, value=1):
    rng = np.random.default_rng(seed * 7919 + H * 131 + W * 17 + int(density * 100))
    return ((rng.random((H, W)) < density) * value).astype(np.uint8)


def serpentine(H=256, W=256):
    """Full even rows joined at alternating ends: one component, a path of about H * W / 2 pixels."""
    m = np.zeros((H, W), np.uint8)
    m[0::2, :] = 1
    m[1::4, W - 1] = 1
    m[3::4, 0] = 1
    return m


def double_spiral(S=255):
    """Two square spiral arms, each the other's half-turn about the centre: equal areas, never touching."""
    m = np.zeros((S, S), np.uint8)
    c = S // 2
    y, x = c, c + 1
    m[y, x] = 1
    dirs = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    seg, d, grow = 1, 0, 3  # segments 1, 4, 7, ...: the half-turned copy runs between the windings, one pixel clear
    while True:
        dy, dx = dirs[d % 4]
        ok = True
        for _ in range(seg):
            y, x = y + dy, x + dx
            if not (0 <= y < S and 0 <= x < S):
                ok = False
                break
            m[y, x] = 1
        if not ok:
            break
        d += 1
        seg += grow
    return (m | m[::-1, ::-1]).astype(np.uint8)


def u_shape(H=256, W=256):
    """Two arms that meet only in the last row: a late merge in raster order."""
    m = np.zeros((H, W), np.uint8)
    m[:, W // 8] = 1
    m[:, W - 1 - W // 8] = 1
    m[H - 1, W // 8:W - W // 8] = 1
    return m


def comb(H=256, W=256, spine_last=False):
    m = np.zeros((H, W), np.uint8)
    m[:, ::2] = 1
    m[H - 1 if spine_last else 0, :] = 1
    return m


def checkerboard(H=256, W=256):
    y, x = np.mgrid[0:H, 0:W]
    return ((y + x) % 2 == 0).astype(np.uint8)


def singletons(H=256, W=256):
    m = np.zeros((H, W), np.uint8)
    m[::2, ::2] = 1
    return m


def borders(H=256, W=256):
    """A component on each corner and each border, of different areas, none touching another."""
    m = np.zeros((H, W), np.uint8)
    m[0, 0] = 1
    m[0, W - 2:] = 1
    m[H - 3:, 0] = 1
    m[H - 2:, W - 2:] = 1
    m[0, W // 2 - 2:W // 2 + 3] = 1
    m[H - 1, W // 2 - 3:W // 2 + 3] = 1
    m[H // 2 - 3:H // 2 + 4, 0] = 1
    m[H // 2 - 4:H // 2 + 4, W - 1] = 1
    return m


def row_wrap(H, W):
    """Pixels at (r, W - 1) and (r + 1, 0) for several r: joined only if the indexing wrapped."""
    m = np.zeros((H, W), np.uint8)
    for r in range(0, H - 1, 3):
        m[r, W - 1] = 1
        m[r + 1, 0] = 1
    return m


def structures():
    """(name, mask, components) of every structure, `components` = the count the oracle must find."""
    return [
        ("serpentine", serpentine(), 1),
        ("serpentine_t", np.ascontiguousarray(serpentine().T), 1),
        ("serpentine_odd", serpentine(37, 53), 1),
        ("double_spiral", double_spiral(), 2),
        ("u_shape", u_shape(), 1),
        ("u_shape_odd", u_shape(37, 53), 1),
        ("comb", comb(), 1),
        ("comb_last", comb(spine_last=True), 1),
        ("checkerboard", checkerboard(), 1),
        ("checkerboard_odd", checkerboard(255, 257), 1),
        ("singletons", singletons(), 16384),
        ("borders", borders(), 8),
        ("row_wrap", row_wrap(256, 256), 2 * len(range(0, 255, 3))),
        ("row_wrap_odd", row_wrap(37, 53), 2 * len(range(0, 36, 3))),
    ]
