"""The numpy restatement of the display transform's rule (include/ptk.h, "display transform"): float32 operation by operation in the
order the header writes them, the histogram and the exposure's rank arithmetic in Python integers.  The sRGB threshold table is an
ARGUMENT - ptk.display_srgb_table() is its definition, nothing here recomputes it.  The GPU tests hold the kernels to these bytes
and to the bits of this state with array_equal."""
import numpy as np

f32 = np.float32
MANUAL, METERED = 0, 1
LINEAR, REINHARD, ACES = 0, 1, 2
T_LINEAR, T_SRGB = 0, 1
BINS = 2048
NO_STATE = dict(exposure=f32(0), target=f32(0), lavg=f32(0), has_prev=0, counted=0, kept=0)


def params(**kw):
    """ptk.display_defaults as a dict"""
    p = dict(mode=METERED, exposure=1.0, key=0.18, min_lum=2.0 ** -20, max_lum=2.0 ** 20, low_permille=100, high_permille=950,
             min_exposure=2.0 ** -10, max_exposure=2.0 ** 10, adapt=1.0, op=ACES, white=4.0, transfer=T_SRGB)
    assert set(kw) <= set(p), kw
    p.update(kw)
    return p


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def luminance(color):
    c = np.asarray(color, f32)
    with np.errstate(all="ignore"):
        return ((f32(0.2126) * c[..., 0]) + (f32(0.7152) * c[..., 1])) + (f32(0.0722) * c[..., 2])


def histogram(color, p):
    """[2048] counts of bits(L) >> 20 over the pixels with min_lum <= L <= max_lum"""
    L = luminance(color).reshape(-1)
    with np.errstate(all="ignore"):
        counted = (L >= f32(p["min_lum"])) & (L <= f32(p["max_lum"]))
    return np.bincount((bits(L[counted]) >> 20).astype(np.int64), minlength=BINS)


def exposure(hist, p, prev=None):
    """the state behind the exposure step over `hist`, given the state `prev` in front of it"""
    prev = NO_STATE if prev is None else prev
    has_prev = bool(prev["has_prev"])
    counts = [int(x) for x in hist]
    N = sum(counts)
    lavg, K = f32(0), 0
    if N > 0:
        lo = N * int(p["low_permille"]) // 1000
        hi = N * int(p["high_permille"]) // 1000
        if hi <= lo:
            hi = lo + 1
        K, S, r = hi - lo, 0, 0
        for b, n in enumerate(counts):
            a, e = max(r, lo), min(r + n, hi)
            if e > a:
                S += (e - a) * b
            r += n
        mbits = ((S << 20) + (K << 19)) // K
        lavg = np.array([mbits], np.uint32).view(f32)[0]
        with np.errstate(all="ignore"):
            target = f32(p["key"]) / lavg
        target = target if target > f32(p["min_exposure"]) else f32(p["min_exposure"])
        target = target if target < f32(p["max_exposure"]) else f32(p["max_exposure"])
    else:
        target = f32(prev["exposure"]) if has_prev else f32(1)
    if not has_prev or f32(p["adapt"]) >= f32(1):
        e = target
    else:
        e_prev = f32(prev["exposure"])
        with np.errstate(all="ignore"):
            e = e_prev + ((target - e_prev) * f32(p["adapt"]))
    return dict(exposure=f32(e), target=f32(target), lavg=f32(lavg), has_prev=1 if (has_prev or N > 0) else 0, counted=N, kept=K)


def apply(color, e, p, table):
    """[..., 3] uint8: exposure e, the tone curve and the encoding over color"""
    c = np.asarray(color, f32)
    table = np.asarray(table, f32)
    assert table.shape == (256,)
    with np.errstate(all="ignore"):
        x = c * f32(e)
        x = np.where(x > 0, x, f32(0))
        if p["op"] == REINHARD:
            iw2 = f32(1) / (f32(p["white"]) * f32(p["white"]))
            y = (x * (f32(1) + (x * iw2))) / (f32(1) + x)
        elif p["op"] == ACES:
            y = (x * ((f32(2.51) * x) + f32(0.03))) / ((x * ((f32(2.43) * x) + f32(0.59))) + f32(0.14))
        else:
            y = x
        y = np.where(y < 1, y, f32(1)).astype(f32)
        if p["transfer"] == T_SRGB:
            return np.searchsorted(table[1:], y, side="right").astype(np.uint8)      # #{ k in 1..255 : T[k] <= y }
        return (y * f32(255)).astype(np.uint8)


def display(color, p, table, prev=None):
    """(bytes, state behind the call): ptk_display_planes over color with the state `prev` in front of it"""
    if p["mode"] == METERED:
        state = exposure(histogram(color, p), p, prev)
        return apply(color, state["exposure"], p, table), state
    return apply(color, f32(p["exposure"]), p, table), (dict(NO_STATE) if prev is None else prev)


def accum_color(s1, counts):
    """PTK_DISPLAY_ACCUM's colour: S1_c / (float)n_p, 0 where n_p = 0; counts [H, W] or one int"""
    s1 = np.asarray(s1, f32)
    n = np.broadcast_to(np.asarray(counts), s1.shape[:2]).astype(np.uint32)
    nf = n.astype(f32)[..., None]
    with np.errstate(all="ignore"):
        return np.where(n[..., None] > 0, s1 / nf, f32(0)).astype(f32)


def state_equal(a, b):
    """bit equality of two states (dicts as Context.display_state gives them)"""
    return (all(bits(a[k]) == bits(b[k]) for k in ("exposure", "target", "lavg"))
            and all(int(a[k]) == int(b[k]) for k in ("has_prev", "counted", "kept")))
