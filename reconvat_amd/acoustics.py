"""Acoustic augmentation of the device feed: every training item is its crop as another room, another microphone and
another noise floor would have recorded it -- one long FIR per item (reverberation convolved with an equaliser) plus white noise.
The labels are untouched.  Sample rate 16 000 Hz.

Definition (everything here, `rv_fir_items` in csrc/acoustics.hip and reconvat_amd/feed.py implement exactly this):

  options  Acoustics(rt60=0.0, eq_db=0.0, noise_db=None, taps=4096): rt60 in [0, 1.0] seconds, eq_db in [0, 12], noise_db None or in
           [-90, -20] dBFS, taps = R a multiple of 16 in [16, 8192] and at least 256 when rt60 > 0; anything else is a ValueError.
           rt60 == 0, eq_db == 0 and noise_db None: the object is "off".
  draws    one stream RandomState(acoustics_seed), per item in item order, the same seven draws in the same order whichever options
           are on (a part that is off ignores its draws):
               u = uniform(0.25, 1.0), rt = rt60 u         drr = uniform(0.0, 12.0)  direct-to-reverberant energy ratio in dB
               n0 = randint(16, 161)  pre-delay, samples   w = standard_normal(R)    g = uniform(-1.0, 1.0, 5)
               un = uniform(0.0, 1.0)                      seed = randint(0, 2**31)
  room     float64 [R]: env[n] = 10^(-3 (n - n0) / (rt 16000)) for n >= n0, else 0; t = w env scaled so that sum t^2 = 10^(-drr / 10);
           room = t with room[0] += 1.  rt60 == 0: the unit impulse.
  eq       63 taps, linear phase, centre tap 31: anchors (0, 250, 1000, 4000, 8000) Hz with gains eq_db g dB; on the 33 bins
           f_i = 250 i: G = 10^(interp(f_i, anchors, gains) / 20), e = irfft(G, 64), eq[j] = e[(j - 31) % 64] hanning(63)[j].
           eq_db == 0: the exact unit impulse at tap 31, nothing designed.
  filter   h = convolve(room, eq) (R + 62 values) zero-padded to W = R + 64, lead = 31: the equaliser's delay is taken out again,
           so the labels stay aligned.
  noise    counter-based, all in uint32 arithmetic with wrap-around:
               lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
               v = lowbias32(seed ^ lowbias32(m + 0x9E3779B9)),  t = (v & 0xFFFF) + (v >> 16) - 65535   (a triangular integer)
               sigma = 10^((noise_db - 20 un) / 20),  amp = float32(sigma sqrt(6) / 65536),  noise[m] = float32(t) * amp
           (one float32 multiply).  noise_db None: amp = 0.
  item     y[m] = sum_{j < W} h[j] x[m + lead - j] + noise[m],  m = 0 .. n - 1,  x zero outside [0, n).

Not modelled: the reverberation starts with the crop -- the tail of what sounded before the crop's first sample is absent, so the
first rt seconds of an item are drier than a real recording's.  The room is exponentially decaying Gaussian noise, not a measured
response; the noise is white.

`apply_item` is the host yardstick (float64, unrounded filter): the only path without a GPU, and what the tests compare with.
"""
import numpy as np

SAMPLE_RATE = 16000
EQ_TAPS = 63
LEAD = 31
ANCHORS = (0.0, 250.0, 1000.0, 4000.0, 8000.0)
MAX_TAPS = 8192


class Acoustics:
    """The options of the augmentation, checked; `off` when nothing is switched on."""

    def __init__(self, rt60=0.0, eq_db=0.0, noise_db=None, taps=4096):
        if isinstance(rt60, bool) or not isinstance(rt60, (int, float)) or not 0.0 <= rt60 <= 1.0:
            raise ValueError(f'rt60 must lie in [0, 1.0] seconds (got {rt60!r})')
        if isinstance(eq_db, bool) or not isinstance(eq_db, (int, float)) or not 0.0 <= eq_db <= 12.0:
            raise ValueError(f'eq_db must lie in [0, 12] dB (got {eq_db!r})')
        if noise_db is not None and (isinstance(noise_db, bool) or not isinstance(noise_db, (int, float)) or not -90.0 <= noise_db <= -20.0):
            raise ValueError(f'noise_db must be None or lie in [-90, -20] dBFS (got {noise_db!r})')
        if isinstance(taps, bool) or not isinstance(taps, (int, np.integer)) or taps % 16 or not 16 <= taps <= MAX_TAPS:
            raise ValueError(f'taps must be a multiple of 16 in [16, {MAX_TAPS}] (got {taps!r})')
        if rt60 > 0 and taps < 256:
            raise ValueError(f'taps must be at least 256 with rt60 > 0 (got {taps!r})')
        self.rt60, self.eq_db, self.taps = float(rt60), float(eq_db), int(taps)
        self.noise_db = None if noise_db is None else float(noise_db)

    @property
    def off(self):
        return self.rt60 == 0.0 and self.eq_db == 0.0 and self.noise_db is None

    @property
    def width(self):
        """W: values of an item's filter."""
        return self.taps + EQ_TAPS + 1

    def __repr__(self):
        return f'Acoustics(rt60={self.rt60}, eq_db={self.eq_db}, noise_db={self.noise_db}, taps={self.taps})'


def draw(aug, acoustics):
    """The parameters of the next item: the seven draws from `aug` in order, and what the options make of them."""
    u = float(aug.uniform(0.25, 1.0))
    drr = float(aug.uniform(0.0, 12.0))
    n0 = int(aug.randint(16, 161))
    w = aug.standard_normal(acoustics.taps)
    g = aug.uniform(-1.0, 1.0, 5)
    un = float(aug.uniform(0.0, 1.0))
    seed = int(aug.randint(0, 2 ** 31))
    if acoustics.noise_db is None:
        amp = np.float32(0.0)
    else:
        sigma = 10.0 ** ((acoustics.noise_db - 20.0 * un) / 20.0)
        amp = np.float32(sigma * np.sqrt(6.0) / 65536.0)
    return {'taps': acoustics.taps, 'rt': acoustics.rt60 * u, 'drr': drr, 'n0': n0, 'w': w, 'eq_db': acoustics.eq_db, 'g': g,
            'un': un, 'seed': seed, 'amp': amp}


def room_filter(params):
    """float64 [R]: the direct sound plus an exponentially decaying Gaussian tail; rt == 0: the unit impulse."""
    R = int(params['taps'])
    room = np.zeros(R)
    if params['rt'] > 0:
        n = np.arange(R, dtype=np.float64)
        n0 = int(params['n0'])
        env = np.where(n >= n0, 10.0 ** (-3.0 * (n - n0) / (params['rt'] * SAMPLE_RATE)), 0.0)
        t = np.asarray(params['w'], dtype=np.float64) * env
        room = t * np.sqrt(10.0 ** (-params['drr'] / 10.0) / np.sum(t * t))
    room[0] += 1.0
    return room


def eq_filter(params):
    """float64 [63]: the windowed linear-phase equaliser through the five anchor gains; eq_db == 0: the unit impulse at tap 31."""
    if params['eq_db'] == 0:
        eq = np.zeros(EQ_TAPS)
        eq[LEAD] = 1.0
        return eq
    gains = params['eq_db'] * np.asarray(params['g'], dtype=np.float64)
    G = 10.0 ** (np.interp(250.0 * np.arange(33), ANCHORS, gains) / 20.0)
    e = np.fft.irfft(G, 64)
    j = np.arange(EQ_TAPS)
    return e[(j - LEAD) % 64] * np.hanning(EQ_TAPS)


def item_filter(params):
    """(h float64 [W], lead): room * eq, zero-padded to W = R + 64."""
    h = np.zeros(int(params['taps']) + EQ_TAPS + 1)
    h[:-2] = np.convolve(room_filter(params), eq_filter(params))
    return h, LEAD


def _lowbias32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def noise(seed, n, amp):
    """float32 [n]: noise[m] = float32(t(seed, m)) * amp, t the triangular integer of the definition."""
    with np.errstate(over='ignore'):
        m = np.arange(int(n), dtype=np.uint32)
        v = _lowbias32(np.uint32(seed) ^ _lowbias32(m + np.uint32(0x9E3779B9)))
    t = (v & np.uint32(0xFFFF)).astype(np.int64) + (v >> np.uint32(16)).astype(np.int64) - 65535
    return t.astype(np.float32) * np.float32(amp)


def apply_item(x, params, magnitude=False):
    """The host yardstick: y[m] = sum_j h[j] x[m + lead - j] + noise[m] in float64 over the item x [n] (zero outside it);
    `magnitude`: S[m] = sum_j |h[j]| |x[m + lead - j]|, without the noise."""
    x = np.asarray(x, dtype=np.float64)
    h, lead = item_filter(params)
    n = len(x)
    if magnitude:
        return np.convolve(np.abs(x), np.abs(h))[lead:lead + n]
    return np.convolve(x, h)[lead:lead + n] + noise(params['seed'], n, params['amp']).astype(np.float64)
