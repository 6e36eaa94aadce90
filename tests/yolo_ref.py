"""The yolo_head contract (include/snnhip.h) in NumPy, float64 or the same expressions in float32, on the head values as stored; an input's three margins;
the GPU tests' inputs: scores from a shuffled, evenly spaced ladder, everything else far below the threshold, geometry from a fixed seed."""
import numpy as np

ANCHORS = (10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319)
MASKS = (3, 4, 5, 1, 2, 3)
# D: the largest fp32-to-float64 distance of a score, a box value (w, h relative) or a tested IoU over CASES; 4 D: the margin of every decision, the row tolerance
D = 1.8e-6
EPS = 4 * D


def params(net=96, n_heads=2, classes=1, conf=0.35, iou=0.45, scale=(32, 16), A=3):
    return dict(net=net, n_heads=n_heads, classes=classes, conf=conf, iou=iou, scale=scale[:n_heads], A=A)


def _geometry(p):
    """per candidate, in candidate order (head, gy, gx, anchor): gx, gy, grid, anchor w, anchor h, float(scale * grid), head"""
    cols = []
    for h, s in enumerate(p["scale"]):
        g = p["net"] // s
        i = np.arange(g * g * p["A"])
        a = np.array(MASKS)[h * p["A"] + i % p["A"]]
        cols.append(np.stack([i // p["A"] % g, i // p["A"] // g, 0 * i + g, np.array(ANCHORS)[2 * a], np.array(ANCHORS)[2 * a + 1], 0 * i + s * g, 0 * i + h], 1))
    return np.concatenate(cols).astype(np.float64).T


def _iou(a, b, f):
    x0, y0 = np.maximum(a[0], b[:, 0]), np.maximum(a[1], b[:, 1])
    x1, y1 = np.minimum(a[0] + a[2], b[:, 0] + b[:, 2]), np.minimum(a[1] + a[3], b[:, 1] + b[:, 3])
    inter = (x1 - x0) * (y1 - y0)
    with np.errstate(all="ignore"):
        return np.where((x1 < x0) | (y1 < y0), f(0), inter / (a[2] * a[3] + b[:, 2] * b[:, 3] - inter))


def decode(heads, p, f=np.float64):
    """One image's heads [g][g][A * (5 + classes)] -> rows [k][6], boxes over the threshold, margins (|prob - conf|, score gap, |iou - thr| tested), IoUs."""
    v = np.concatenate([np.asarray(h).reshape(-1, 5 + p["classes"]) for h in heads]).astype(f)
    gx, gy, g, aw, ah, ext, _ = _geometry(p).astype(f)
    one, conf, thr = f(1), f(np.float32(p["conf"])), f(np.float32(p["iou"]))
    cls = np.argmax(v[:, 5:], 1)  # the first maximum
    prob = one / (one + np.exp(-v[:, 4]) * (one + np.exp(-v[:, 5:].max(1))))
    k = np.flatnonzero(prob > conf)
    k = k[np.argsort(-prob[k], kind="stable")]
    sig = lambda t: one / (one + np.exp(-t))
    w, h = np.exp(v[k, 2]) * aw[k] / ext[k], np.exp(v[k, 3]) * ah[k] / ext[k]
    box = np.stack([(gx[k] + sig(v[k, 0])) / g[k] - w / f(2), (gy[k] + sig(v[k, 1])) / g[k] - h / f(2), w, h], 1)
    merged, kept, ious = np.zeros(len(k), bool), [], [np.zeros(0, f)]
    for i in range(len(k)):
        if not merged[i]:
            j = i + 1 + np.flatnonzero(~merged[i + 1:] & (cls[k[i + 1:]] == cls[k[i]]))
            ious.append(_iou(box[i], box[j], f))
            merged[j[ious[-1] > thr]] = True
            kept.append(i)
    rows = np.concatenate([np.stack([cls[k], prob[k]], 1).astype(f), box], 1)[kept].reshape(-1, 6)
    gaps, ious = -np.diff(prob[k]), np.concatenate(ious)
    margins = (np.abs(prob - conf).min(), gaps[gaps > 0].min(initial=np.inf), np.abs(ious - thr).min(initial=np.inf))
    return rows, len(k), margins, ious


def distance(heads, p):
    """the fp32-to-float64 distance of the rows (w, h relative) and of the tested IoUs; the two evaluations must take the same decisions"""
    (r64, n64, _, i64), (r32, n32, _, i32) = decode(heads, p), decode(heads, p, np.float32)
    assert r64.shape == r32.shape and n64 == n32 and i64.shape == i32.shape and np.array_equal(r64[:, 0], r32[:, 0])
    d = np.abs(r64 - r32)
    d[:, 4:] /= r64[:, 4:]
    return max(d.max(initial=0), np.abs(i64 - i32).max(initial=0))


def make_image(p, count, mode, seed, ties=False, dtype=np.float32):
    """One image's heads: `count` survivors ("all": every candidate) with ladder scores; mode "small": boxes too small to meet, "overlap": anchor-sized."""
    rng = np.random.default_rng(seed)
    geo = _geometry(p)
    M, K = geo.shape[1], geo.shape[1] if count == "all" else count
    v = np.full((M, 5 + p["classes"]), -12.0)
    v[:, 5:] = 0.0
    pick = np.sort(rng.choice(M, K, replace=False))
    v[pick, 5 + rng.integers(0, p["classes"], K)] = 2.0
    if p["classes"] > 1 and K:
        v[pick[0], 5:7] = 2.0  # a tie of the class logits: the first wins
    v[pick, 4] = -np.log((1 / rng.permutation(np.linspace(0.40, 0.95, K)) - 1) / (1 + np.exp(-2.0)))
    if mode == "small":  # anchors of a cell side by side, the two heads on rows of their own, sizes below 3e-4
        centre = np.stack([0.25 * (pick % p["A"] + 1), 0.3 + 0.4 * geo[6, pick]], 1)
        v[pick, :4] = np.concatenate([np.log(centre / (1 - centre)) + rng.normal(0, 0.01, (K, 2)), rng.normal(-8, 0.1, (K, 2))], 1)
    else:
        v[pick, :4] = np.concatenate([rng.normal(0, 1, (K, 2)), rng.normal(0, 0.3, (K, 2))], 1)
    if ties:  # identical logits in two cells of the first head and in one of the last: equal scores, candidate order decides
        v[pick[1]] = v[pick[-1]] = v[pick[0]]
    cut = np.cumsum([0] + [(p["net"] // s) ** 2 * p["A"] for s in p["scale"]])
    return [v[a:b].reshape(p["net"] // s, p["net"] // s, -1).astype(dtype) for a, b, s in zip(cut, cut[1:], p["scale"])]


# name: (params, [(count, mode, seed, ties)] per image, storage dtype, max_boxes or None = every candidate)
CASES = {
    "net32_none": (params(32), [(0, "small", 1, False)], np.float32, None),
    "net32_one": (params(32), [(1, "small", 2, False)], np.float32, None),
    "net96_65": (params(96), [(65, "overlap", 3, False)], np.float32, None),
    "net96_all": (params(96), [("all", "small", 4, False)], np.float32, None),
    "net416_all_apart": (params(416), [("all", "small", 5, False)], np.float32, None),
    "net416_all_overlap": (params(416), [("all", "overlap", 6, False)], np.float32, None),
    "net96_ties": (params(96), [(40, "overlap", 7, True)], np.float32, None),
    "net96_max_boxes": (params(96), [(65, "small", 8, False)], np.float32, 10),
    "net96_three_images": (params(96), [(65, "overlap", 9, False), (0, "small", 10, False), (20, "overlap", 11, False)], np.float32, None),
    "net96_one_head": (params(96, n_heads=1), [(10, "overlap", 12, False)], np.float32, None),
    "net96_three_classes": (params(96, classes=3), [(60, "overlap", 13, False)], np.float32, None),
    "net96_fp16": (params(96), [(65, "overlap", 14, False)], np.float16, None),
    "net96_three_classes_fp16": (params(96, classes=3), [(60, "overlap", 15, False)], np.float16, None),
}


def case_images(name):
    p, images, dtype, _ = CASES[name]
    return [make_image(p, c, m, s, t, dtype) for c, m, s, t in images]
