"""The Halton sampler in exact integer / rational arithmetic: the helpers tests/test_halton.py holds the oracle's sampler to, and the
sampler's value of any dimension >= 2 at any pixel sample -- what tests/direct_cases.py holds an implementation's sampler hook to before the
direct-lighting truth takes the hook's float32 numbers as its inputs.  Numpy-free, independent of the oracle and of the product."""
from fractions import Fraction

K_MAX_RESOLUTION = 128


class Pcg32:
    """core/rng.rs:8-67 (scalar; only used for the small shuffles below)."""
    M = (1 << 64) - 1

    def __init__(self, seq=None):
        self.state, self.inc = 0x853c49e6748fea9b, 0xda3e39cb94b95bdb
        if seq is not None:
            self.state, self.inc = 0, ((seq << 1) | 1) & self.M
            self.u32()
            self.state = (self.state + 0x853c49e6748fea9b) & self.M
            self.u32()

    def u32(self):
        old = self.state
        self.state = (old * 0x5851f42d4c957f2d + self.inc) & self.M
        xs = (((old >> 18) ^ old) >> 27) & 0xffffffff
        rot = old >> 59
        return ((xs >> rot) | (xs << ((-rot) & 31))) & 0xffffffff

    def below(self, b):
        threshold = ((1 << 32) - b) % b
        while True:
            r = self.u32()
            if r >= threshold:
                return r % b


def shuffle(a, rng):
    """shuffle_array with one dimension (core/sampling/sampling.rs:4-15)."""
    n = len(a)
    for i in range(n):
        other = i + rng.below(n - i)
        a[i], a[other] = a[other], a[i]


def primes(n):
    out, c = [], 2
    while len(out) < n:
        if all(c % p for p in out if p * p <= c):
            out.append(c)
        c += 1
    return out


def default_permutations(n_dims):
    """compute_radical_inverse_permutations with RNG::new() (halton.rs:12-20, radical_inverse.rs:111-129): one shuffle per prime, all drawn
    from the same default-state stream, identity start."""
    rng = Pcg32()
    out = []
    for p in primes(n_dims):
        a = list(range(p))
        shuffle(a, rng)
        out.append(a)
    return out


def scrambled_radical_inverse(base, perm, index):
    """sum perm[d_i] b^-(i+1) + perm[0] b^-n / (b - 1), exactly."""
    digits = []
    while index:
        digits.append(index % base)
        index //= base
    v = sum(Fraction(int(perm[d]), base ** (i + 1)) for i, d in enumerate(digits))
    return v + Fraction(int(perm[0]), base ** len(digits) * (base - 1))


def _reversed_digits(v, base, n):
    out = 0
    for _ in range(n):
        out, v = out * base + v % base, v // base
    return out


def pixel_sample_index(sample_bounds, px, py, n):
    """get_index_for_sample (halton.rs:115-147) by what it is for: the index whose first two dimensions, scaled to the 2^e0 x 3^e1 tile that
    covers min(resolution, 128), land in pixel (px, py) mod 128 -- its lowest e0 binary (e1 ternary) digits are the pixel coordinate's,
    reversed -- plus n strides."""
    res = (sample_bounds[2] - sample_bounds[0], sample_bounds[3] - sample_bounds[1])
    scale, exp = [1, 1], [0, 0]
    for i, base in enumerate((2, 3)):
        while scale[i] < min(res[i], K_MAX_RESOLUTION):
            scale[i] *= base
            exp[i] += 1
    stride = scale[0] * scale[1]
    want = [_reversed_digits((p % K_MAX_RESOLUTION) % scale[i], b, exp[i]) for i, (p, b) in enumerate(((px, 2), (py, 3)))]
    offset = next(o for o in range(stride) if o % scale[0] == want[0] and o % scale[1] == want[1])
    return offset + n * stride
