"""numpy restatement of the Canny definition written out in include/ltx2hip.h (OpenCV's Canny with apertureSize 3 and L2gradient false, to
the best of our knowledge: no OpenCV binary was at hand), and of the uint8 -> patchified-operand glue.  Checker side only: nothing here is
imported by the package.  The hysteresis exists twice, by flood fill and by connected-component labelling; the tests hold them equal."""
import numpy as np


def gray(rgb):
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))
    return (r * 9798 + g * 19235 + b * 3735 + 16384) >> 15


def sobel(g):
    """3x3 Sobel gx, gy of an integer image (H, W) with a replicated border."""
    p = np.pad(g.astype(np.int32), 1, mode="edge")
    a, b, c = p[:-2, :-2], p[:-2, 1:-1], p[:-2, 2:]
    d, e = p[1:-1, :-2], p[1:-1, 2:]
    f, h, k = p[2:, :-2], p[2:, 1:-1], p[2:, 2:]
    return (c + 2 * e + k) - (a + 2 * d + f), (f + 2 * h + k) - (a + 2 * b + c)


def thresholds(low, high):
    lo, hi = int(np.floor(low)), int(np.floor(high))
    return (hi, lo) if lo > hi else (lo, hi)


def canny_map(rgb, low, high):
    """One frame (H, W, 3) uint8 -> map (H, W) uint8 of {0, 1 = weak, 2 = strong}."""
    lo, hi = thresholds(low, high)
    gx, gy = sobel(gray(rgb))
    mag = np.abs(gx) + np.abs(gy)
    m = np.pad(mag, 1)                                   # 0 outside the image
    H, W = mag.shape
    at = lambda dy, dx: m[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    x, y = np.abs(gx), np.abs(gy) << 15
    t22 = x * 13573
    t67 = t22 + (x << 16)
    horiz = y < t22
    vert = ~horiz & (y > t67)
    diag = ~horiz & ~vert
    neg = (gx ^ gy) < 0                                  # s = -1: compare with (y-1, x+1) and (y+1, x-1)
    keep = (horiz & (mag > at(0, -1)) & (mag >= at(0, 1))) | (vert & (mag > at(-1, 0)) & (mag >= at(1, 0))) | \
        (diag & neg & (mag > at(-1, 1)) & (mag > at(1, -1))) | (diag & ~neg & (mag > at(-1, -1)) & (mag > at(1, 1)))
    keep &= mag > lo
    return np.where(keep, np.where(mag > hi, 2, 1), 0).astype(np.uint8)


def hysteresis_flood(cmap):
    """One map (H, W) -> edges (H, W) uint8 {0, 255}: a stack-based flood fill from every strong pixel."""
    H, W = cmap.shape
    out = np.zeros((H, W), np.uint8)
    stack = [tuple(p) for p in np.argwhere(cmap == 2)]
    for p in stack:
        out[p] = 255
    while stack:
        y, x = stack.pop()
        for yy in range(max(y - 1, 0), min(y + 2, H)):
            for xx in range(max(x - 1, 0), min(x + 2, W)):
                if cmap[yy, xx] and not out[yy, xx]:
                    out[yy, xx] = 255
                    stack.append((yy, xx))
    return out


def hysteresis_label(cmap):
    """The same by connected components: 8-connected components of map != 0 that hold a strong pixel."""
    from scipy import ndimage
    lab, _ = ndimage.label(cmap != 0, structure=np.ones((3, 3), np.int32))
    good = np.unique(lab[cmap == 2])
    return (np.isin(lab, good[good != 0]) * 255).astype(np.uint8)


def hysteresis(cmaps):
    """(F, H, W) maps -> (F, H, W) edges; frames are independent."""
    return np.stack([hysteresis_label(m) for m in cmaps])


def canny(frames, low, high):
    """(F, H, W, 3) uint8 -> (F, H, W) uint8 {0, 255}."""
    return hysteresis(np.stack([canny_map(f, low, high) for f in frames]))


def serpentine(h, w):
    """A one-pixel path of weak pixels (1) that covers an (h, w) map: every second row in full, joined at alternating ends.  Returns the map
    and the (y, x) of the path's first pixel."""
    m = np.zeros((h, w), np.uint8)
    m[0::2] = 1
    for i, y in enumerate(range(1, h, 2)):
        if y + 1 < h:
            m[y, w - 1 if i % 2 == 0 else 0] = 1
    return m, (0, 0)
