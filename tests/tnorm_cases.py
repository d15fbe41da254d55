"""The normalisation pass restated in float64 numpy (src/TNormCu.cc:262-327), and the case tables of its tests
(tests/test_tnorm_cpu.py, tests/test_gpu_tnorm.py, tests/golden/make_tnorm.py).

The reference, per utterance, after the transform and the trim of the context rows:
    BaseFloat val = feats(m, n);  first[n] += val;  second[n] += val * val;          (:262-267)
val * val is a float product, rounded to float, then widened to the double accumulator.  framesN grows by
feats_host.Rows(): the rows INCLUDING the STARTFRMEXT + ENDFRMEXT context rows (:286), although only the trimmed rows
were summed -- the frame-count quirk (count_ext_frames=True); count_ext_frames=False divides by the summed rows.  Then
    mean = first / N;  variance = second / N - mean^2;  bias = -mean;  window = 1 / sqrt(variance)      (:298-317)
and the file (:320-327): "<bias> D D\\n" + bias + "\\n\\n" + "<window> D D\\n" + window + "\\n\\n", a vector being
"v D  " and every element followed by a blank (Vector.tcc:550-571) at the stream's default precision: 6 significant
digits of the DOUBLE ("%g").
"""
import numpy as np

# ---- kernel case tables (tests/test_gpu_tnorm.py adds the kernel's own slab height R and slot count S)
EXACT_ROWS = (1, 2, 63, 64, 65)
EXACT_COLS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 598, 1173)
EXACT_MAX = 1024            # integer inputs |x| <= 1024: x*x <= 2^20 is exact in fp32, every sum exact in double
VIEW_SHAPES = ((37, 64), (37, 65), (130, 260), (33, 598))
# examples/01 at the recipe's frame extension
EX01_EXT = 25
EX01_FRAMES = 55457         # summed frames
EX01_FRAMES_EXT = 60457     # + 100 utterances x 50 context rows: the reference's N


def exact_rows(R, S):
    """the row counts of the exact cases for slab height R and S slots"""
    return tuple(dict.fromkeys(EXACT_ROWS + (R - 1, R, R + 1, S * R + 1)))


def moments(y):
    """(first, second, abs_sum) of one trimmed utterance y [rows x D] (float32): the fp32 square, then double sums"""
    y = np.ascontiguousarray(y, np.float32)
    sq = y * y                                   # float32 product, rounded to float32
    return (y.astype(np.float64).sum(0), sq.astype(np.float64).sum(0), np.abs(y).astype(np.float64).sum(0))


class Accumulator:
    """TNormCu's loop state over trimmed utterances"""

    def __init__(self, dim, start_ext=0, end_ext=0, count_ext_frames=True):
        self.first, self.second, self.abs_sum = (np.zeros(dim, np.float64) for _ in range(3))
        self.ext = start_ext + end_ext
        self.count_ext_frames = count_ext_frames
        self.frames = 0      # N of the division
        self.summed = 0      # rows that entered the sums

    def add(self, y_trimmed):
        f, s, a = moments(y_trimmed)
        self.first += f
        self.second += s
        self.abs_sum += a
        rows = y_trimmed.shape[0]
        self.summed += rows
        self.frames += rows + self.ext if self.count_ext_frames else rows


def finish(first, second, frames):
    """(bias, window) in double, operation for operation TNormCu.cc:298-317"""
    scale = 1.0 / float(frames)
    mean = np.asarray(first, np.float64) * scale
    variance = np.asarray(second, np.float64) * scale
    variance = variance - mean * mean
    with np.errstate(divide="ignore", invalid="ignore"):
        window = 1.0 / np.sqrt(variance)
    return mean * -1.0, window


def fmt_double(x):
    """operator<<(ostream&, double) at the default precision: printf("%g")"""
    x = float(x)
    if np.isnan(x):
        return "-nan" if np.signbit(x) else "nan"
    return "%g" % x


def fmt_vector(v):
    return "v %d  " % len(v) + "".join(fmt_double(x) + " " for x in v)


def norm_text(bias, window):
    d = len(bias)
    return ("<bias> %d %d\n" % (d, d) + fmt_vector(bias) + "\n\n" + "<window> %d %d\n" % (d, d) + fmt_vector(window) +
            "\n\n")


def report(frames, bias, window):
    return "frames: %d, max_bias: %s, max_window: %s, min_window: %s\n" % (
        frames, fmt_double(np.max(bias)), fmt_double(np.max(window)), fmt_double(np.min(window)))
