"""Canonical rule C10 restated in numpy: the red-object rectangle of the colour branch.

rgb8 image -> 8-bit HSV (H in 0..179, integers only) -> red mask -> 9x9 opening -> 8-connected components -> outer border
of each (Suzuki-Abe border following through pixel centres) -> contourArea as `area2` = 2 * area -> the largest component
(ties: first raster pixel first) -> its pixel bounds grown by the margin, not clipped.

This is the CPU yardstick of `cd_color_bbox_batch`: written from the rule, step by step, sharing no code with the device
path.  Parity with a real OpenCV build is unpinned (OpenCV is not a dependency); the semantics are those of OpenCV 3.x's
8-bit paths as rule C10 states them.
"""
import numpy as np

DEFAULT_PARAMS = {"h_lo_max": 10, "h_hi_min": 175, "s_min": 50, "v_min": 100, "margin": 10}

# direction d of the 8-neighbourhood, clockwise on the screen (x right, y down), starting east: (dx, dy)
_DIRS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))


def _tables():
    i = np.arange(1, 256, dtype=np.float64)
    sdiv = np.zeros(256, np.int64)
    hdiv = np.zeros(256, np.int64)
    sdiv[1:] = np.rint((255 << 12) / i).astype(np.int64)   # np.rint rounds half to even
    hdiv[1:] = np.rint((180 << 12) / (6.0 * i)).astype(np.int64)
    return sdiv, hdiv


SDIV, HDIV = _tables()


def _params(params):
    p = dict(DEFAULT_PARAMS)
    if params is not None:
        if isinstance(params, dict):
            p.update(params)
        else:   # a ctypes cd_color_gate_params
            for k in DEFAULT_PARAMS:
                p[k] = int(getattr(params, k))
    return p


def hsv8(rgb):
    """(..., 3) uint8 rgb -> (h, s, v) int arrays, rule C10 step 1."""
    a = np.asarray(rgb).astype(np.int64)
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    s = (diff * SDIV[v] + 2048) >> 12
    h0 = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h0 * HDIV[diff] + 2048) >> 12   # numpy's >> on signed integers is arithmetic
    h = np.where(h < 0, h + 180, h)
    return h, s, v


def mask(rgb, params=None):
    """Step 2: bool (H, W)."""
    p = _params(params)
    h, s, v = hsv8(rgb)
    return ((h <= p["h_lo_max"]) | (h >= p["h_hi_min"])) & (s >= p["s_min"]) & (v >= p["v_min"])


def _window_all(m, outside):
    """9x9 window reduction: all() for outside = True (erosion), any() for outside = False (dilation)."""
    H, W = m.shape
    pad = np.full((H + 8, W + 8), outside, bool)
    pad[4:4 + H, 4:4 + W] = m
    out = np.full((H, W), outside, bool)
    for dy in range(9):
        for dx in range(9):
            win = pad[dy:dy + H, dx:dx + W]
            out = (out & win) if outside else (out | win)
    return out


def opening(m):
    """Step 3: one 9x9 erosion (outside counts as set) then one 9x9 dilation (outside counts as clear)."""
    m = np.asarray(m, bool)
    return _window_all(_window_all(m, True), False)


def components(m):
    """Step 4, first half: 8-connected components of a bool image.  Returns (labels, comps): labels int32 (H, W), 0 =
    background, components numbered from 1 in the raster order of their first pixel; comps[k - 1] = dict(first = (x, y),
    x0, y0, x1, y1 (inclusive pixel bounds), n = pixels)."""
    m = np.asarray(m, bool)
    H, W = m.shape
    labels = np.zeros((H, W), np.int32)
    comps = []
    ys, xs = np.nonzero(m)
    for y, x in zip(ys.tolist(), xs.tolist()):   # raster order
        if labels[y, x]:
            continue
        k = len(comps) + 1
        labels[y, x] = k
        stack = [(x, y)]
        x0 = x1 = x
        y0 = y1 = y
        n = 0
        while stack:
            cx, cy = stack.pop()
            n += 1
            x0, x1, y0, y1 = min(x0, cx), max(x1, cx), min(y0, cy), max(y1, cy)
            for dx, dy in _DIRS:
                nx, ny = cx + dx, cy + dy
                if 0 <= nx < W and 0 <= ny < H and m[ny, nx] and not labels[ny, nx]:
                    labels[ny, nx] = k
                    stack.append((nx, ny))
        comps.append({"first": (x, y), "x0": x0, "y0": y0, "x1": x1, "y1": y1, "n": n})
    return labels, comps


def _follow(m, start, d_first):
    """Suzuki-Abe border following from `start`, whose neighbour in direction d_first is clear: the first search runs clockwise from there, the walk counter-clockwise.  Returns the closed walk as
    a list of (x, y) (the closing edge back to the first point is implied)."""
    H, W = m.shape

    def at(x, y):
        return 0 <= x < W and 0 <= y < H and bool(m[y, x])

    sx, sy = start
    d1 = None
    for k in range(1, 8):
        d = (d_first + k) & 7
        if at(sx + _DIRS[d][0], sy + _DIRS[d][1]):
            d1 = d
            break
    if d1 is None:
        return [start]
    last = (sx + _DIRS[d1][0], sy + _DIRS[d1][1])   # the walk ends here, one step before it is back at the start
    pts = []
    cur, d_prev = start, d1   # d_prev: direction from cur to the previous point
    while True:
        pts.append(cur)
        for k in range(1, 9):
            d = (d_prev - k) & 7
            nxt = (cur[0] + _DIRS[d][0], cur[1] + _DIRS[d][1])
            if at(*nxt):
                break
        if nxt == start and cur == last:
            return pts
        cur, d_prev = nxt, (d + 4) & 7


def outer_border(m, first):
    """Step 4, second half: the outer border of the component whose first raster pixel is `first` = (x, y): the pixel west
    of it is clear (direction 4)."""
    return _follow(np.asarray(m, bool), tuple(first), 4)


def hole_borders(m):
    """The hole borders RETR_LIST also returns (for the test of rule 4's argument): one walk per hole, started at the
    foreground pixel west of the hole's first raster pixel, whose east neighbour (direction 0) is clear."""
    m = np.asarray(m, bool)
    H, W = m.shape
    bg = np.ones((H + 2, W + 2), bool)
    bg[1:-1, 1:-1] = ~m
    # holes = 4-connected background components that do not reach the frame around the image
    lab = np.zeros(bg.shape, np.int32)
    out = []
    for y0 in range(H + 2):
        for x0 in range(W + 2):
            if not bg[y0, x0] or lab[y0, x0]:
                continue
            k = int(lab.max()) + 1
            lab[y0, x0] = k
            stack = [(x0, y0)]
            while stack:
                cx, cy = stack.pop()
                for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                    nx, ny = cx + dx, cy + dy
                    if 0 <= nx < W + 2 and 0 <= ny < H + 2 and bg[ny, nx] and not lab[ny, nx]:
                        lab[ny, nx] = k
                        stack.append((nx, ny))
            if k > 1:   # (component 1 is the outside: it holds the frame's corner)
                # the hole's first raster pixel is (x0 - 1, y0 - 1) in image coordinates; the pixel west of it is foreground
                out.append(_follow(m, (x0 - 2, y0 - 1), 0))
    return out


def area2(pts):
    """|shoelace sum| of a closed walk = 2 * contourArea, an integer."""
    s = 0
    n = len(pts)
    for i in range(n):
        xa, ya = pts[i]
        xb, yb = pts[(i + 1) % n]
        s += xa * yb - xb * ya
    return abs(s)


def color_bbox(rgb, params=None):
    """Rule C10 on one (H, W, 3) uint8 image -> dict(rect = (x1, y1, x2, y2), found, area2, n_components, n_mask)."""
    p = _params(params)
    m = opening(mask(rgb, p))
    _, comps = components(m)
    out = {"rect": (0, 0, 0, 0), "found": 0, "area2": 0, "n_components": len(comps), "n_mask": int(m.sum())}
    best = None
    for c in comps:   # raster order of the first pixels: a strict '>' keeps the earliest on a tie
        a = area2(outer_border(m, c["first"]))
        if best is None or a > best[0]:
            best = (a, c)
    if best is not None:
        a, c = best
        d = p["margin"]
        x, y, w, h = c["x0"], c["y0"], c["x1"] - c["x0"] + 1, c["y1"] - c["y0"] + 1
        out.update(rect=(x - d, y - d, x + w + d, y + h + d), found=1, area2=int(a))
    return out


def gate_rects(frames, params=None):
    """(F, H, W, 3) uint8 -> (F, 4) int32 rectangles, (0, 0, 0, 0) where no component was found."""
    return np.array([color_bbox(f, params)["rect"] for f in frames], np.int32).reshape(-1, 4)
