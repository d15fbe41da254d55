"""The forward pass restated in float64 / plain Python, and the cases its tests share (tests/test_feacat_cpu.py,
tests/test_gpu_feacat.py).

  mode_fn(y, mode)            TFeaCatCu.cc:244-259: GMMBYPASS y <- (float) sqrt(-2.0 * log(y)), then LOGPOSTERIOR
                              y <- (float) log(y); fp64 from the fp32 input, one rounding per step (the C log(double) /
                              sqrt(double): tests/golden/feacat_ref.npz is reproduced bit for bit, test_feacat_cpu.py)
  emit(Y, segs, mode, swap, out)   the segment scatter of tnet_feacat_emit into a flat uint32 image
  plan(lengths, pack_rows)    which rows of which utterance land where in which pack
  make_htk_file_name(...)     MakeHtkFileName (Common.cc:118-172)
"""
import numpy as np

GMMBYPASS, LOGPOSTERIOR = 1, 2
MODES = (0, GMMBYPASS, LOGPOSTERIOR, GMMBYPASS | LOGPOSTERIOR)
MODE_NAMES = {0: "none", GMMBYPASS: "gmmbypass", LOGPOSTERIOR: "logposterior", GMMBYPASS | LOGPOSTERIOR: "both"}

# the issue's special inputs; the smallest denormal is 2^-149
SPECIALS = np.array([0.0, -0.0, 1.0, 2.0 ** -149, -0.5, np.nan, np.inf], np.float32)


def mode_fn(y, mode):
    y = np.asarray(y, np.float32)
    with np.errstate(all="ignore"):
        if mode & GMMBYPASS:
            y = np.sqrt(-2.0 * np.log(y.astype(np.float64))).astype(np.float32)
        if mode & LOGPOSTERIOR:
            y = np.log(y.astype(np.float64)).astype(np.float32)
    return y


def ulp_distance(a, b):
    """distance in fp32 units in the last place between finite a and b (same shape): the difference of their
    positions on the ordered line of floats"""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def same_footprint(a, b):
    """positions of NaN, positions and signs of +-inf and +-0 agree (a NaN's own sign and payload carry nothing)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    for special in (np.isinf, lambda x: x == 0):
        ma, mb = special(a), special(b)
        if not np.array_equal(ma, mb) or not np.array_equal(np.signbit(a[ma]), np.signbit(b[mb])):
            return False
    return True


def emit(Y, segs, mode, swap, out):
    """segs: [(src_row, dst_row, rows)]; out: flat uint32 image, written in place at word dst_row * C"""
    Y = np.asarray(Y, np.float32)
    C = Y.shape[1]
    for src, dst, rows in segs:
        w = mode_fn(Y[src:src + rows], mode).view(np.uint32).reshape(-1)
        out[dst * C:(dst + rows) * C] = w.byteswap() if swap else w
    return out


def draw_inputs(rng, rows, cols):
    """posterior-like values in (0, 1] with the special values sprinkled in (at least one of each where there is
    room)"""
    Y = (1.0 - rng.random((rows, cols))).astype(np.float32)  # (0, 1]
    flat = Y.reshape(-1)
    n = min(flat.size, 3 * len(SPECIALS))
    where = rng.choice(flat.size, n, replace=False)
    flat[where] = np.resize(SPECIALS, n)
    return Y


def plan(lengths, pack_rows):
    """The packing plan of a row-wise network: utterances (lengths = rows WITHOUT the context rows) back to back,
    a pack closed when it holds pack_rows rows.  Returns [pack] with pack = [(utt, utt_row, pack_row, rows)]."""
    packs, cur, fill = [], [], 0
    for u, n in enumerate(lengths):
        done = 0
        while done < n:
            take = min(n - done, pack_rows - fill)
            cur.append((u, done, fill, take))
            fill += take
            done += take
            if fill == pack_rows:
                packs.append(cur)
                cur, fill = [], 0
    if cur:
        packs.append(cur)
    return packs


def make_htk_file_name(logical, out_dir, out_ext):
    if logical == "-":
        return "-"
    slash = logical.rfind("/")
    base = 0 if slash < 0 else slash + 1
    bend = -1
    if out_ext is not None:
        bend = logical.rfind(".")
    if bend < base:            # no '.', or only in a directory name
        bend = len(logical)
    dots = logical.find("/./")
    if dots >= 0:
        base = dots + 3
    out = ""
    if out_dir is not None:
        if out_dir:
            out += out_dir + "/"
        out += logical[base:bend]
    else:
        out += logical[:bend]
    if out_ext:
        out += "." + out_ext
    return out


# (logical, dir, ext) -> the reference's result, worked out by hand from Common.cc:118-172
FILE_NAME_CASES = [
    (("features/001.fea", "out", "fea"), "out/001.fea"),
    (("/abs/path/utt.one.fbank", "o", "post"), "o/utt.one.post"),
    (("a/./b/c.fea", "out", "fea"), "out/b/c.fea"),          # the /./ rule keeps the directories after it
    (("noext", "out", "fea"), "out/noext.fea"),
    (("dir.d/noext", "out", "fea"), "out/noext.fea"),         # a '.' in a directory name is no extension
    (("x/y.fea", "", "fea"), "y.fea"),                        # an empty directory: the base name alone
    (("x/y.fea", None, "post"), "x/y.post"),                  # no directory: next to the input
    (("x/y.fea", "out", ""), "out/y"),                        # an empty extension strips the old one
    (("x/y.fea", "out", None), "out/y.fea"),                  # no extension: the name as it is
    (("-", "out", "fea"), "-"),
]
