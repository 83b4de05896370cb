"""numpy model of the noise sources and the AWGN channel (csdr_amd/csrc/noise_dev.hpp): integer Philox4x32-10, the reference's words-to-samples
transform evaluated in float64 (get_random_samples_f / get_random_gaussian_samples_c libcsdr.c:2444-2466), the gain formula and the block cycling of
`csdr awgn_cc <snr_db> --awgnfile F` (csdr.c:3035-3091), and normalized_timing_variance_u32_f (libcsdr.c:2293-2317)."""
import numpy as np

f32, f64, u32, u64, c64 = np.float32, np.float64, np.uint32, np.uint64, np.complex64
GAUSSIAN, UNIFORM = 0, 1
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = u64(0xFFFFFFFF)

# Variance of one part (I or Q) of the transform's own distribution: below 1 because u_0 >= 1e-8 clamps r at 6.07 and 0.49999999 narrows u.  From the
# float64 transform over 2^24 Philox words (2^23 samples, seed 0, stream 0), I and Q pooled: measured_v0() below.  Its own sampling error is
# sqrt(2 / 2^24) = 3.5e-4 relative, well inside the 5 sigma gate of 2^20 samples (6.9e-3) that uses it.
V0 = 0.99996


def philox4x32_10(ctr, key):
    """ctr: [..., 4], key: [..., 2] unsigned words -> [..., 4] uint32"""
    c = [np.asarray(ctr)[..., k].astype(u64) for k in range(4)]
    k0, k1 = (np.asarray(key)[..., k].astype(u64) for k in range(2))
    for _ in range(10):
        p0, p1 = u64(M0) * c[0], u64(M1) * c[2]
        c = [(p1 >> u64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> u64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + u64(W0)) & MASK, (k1 + u64(W1)) & MASK
    return np.stack(c, -1).astype(u32)


def blocks(kind, seed, stream_id, j):
    """block(kind, s, j) for an array of block indexes j -> [len(j), 4] words"""
    j = np.asarray(j, u64)
    ctr = np.stack([j & MASK, j >> u64(32), np.full(j.shape, stream_id, u64), np.full(j.shape, kind, u64)], -1)
    key = np.array([int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF], u64)
    return philox4x32_10(ctr, np.broadcast_to(key, j.shape + (2,)))


def gaussian_words(seed, stream_id, position, n):
    """the 2 n words of Gaussian samples position .. position + n - 1 (the reference's pioutput[2 i], pioutput[2 i + 1])"""
    i = np.arange(n, dtype=u64) + u64(position)
    b = blocks(GAUSSIAN, seed, stream_id, i >> u64(1))
    h = (i & u64(1)).astype(np.int64) * 2
    r = np.arange(n)
    return np.stack([b[r, h], b[r, h + 1]], -1).reshape(-1)


def uniform_words(seed, stream_id, position, n):
    k = np.arange(n, dtype=u64) + u64(position)
    b = blocks(UNIFORM, seed, stream_id, k >> u64(2))
    return b[np.arange(n), (k & u64(3)).astype(np.int64)]


def uniform_from_words(w):
    """(float)(int)w / 2147483648.0f: exact"""
    return (np.asarray(w, u32).view(np.int32).astype(f32) / f32(2147483648.0)).astype(f32)


def unit_from_words(w):
    """u_k = (float)(0.5 + 0.49999999 * (double)((float)w / 2147483648.0f))"""
    return (0.5 + 0.49999999 * uniform_from_words(w).astype(f64)).astype(f32)


def gaussian_from_words(w):
    """2 n words -> n complex128 samples: the float32 u_0, u_1 of the reference, everything after them in float64"""
    u = unit_from_words(w).astype(f64).reshape(-1, 2)
    r = np.sqrt(-2.0 * np.log(u[:, 0]))
    return r * np.cos(2 * np.pi * u[:, 1]) + 1j * r * np.sin(2 * np.pi * u[:, 1])


def gaussian(seed, stream_id, position, n):
    return gaussian_from_words(gaussian_words(seed, stream_id, position, n))


def uniform(seed, stream_id, position, n):
    return uniform_from_words(uniform_words(seed, stream_id, position, n))


def measured_v0(n_words=1 << 24):
    g = gaussian(0, 0, 0, n_words // 2)
    return float(np.concatenate([g.real, g.imag]).var())


def awgn_gains(snr_db):
    """(a_signal, a_noise * 0.707 as float) of awgn_cc <snr_db>, csdr.c:3050-3052 and :3079"""
    spn = f32(np.power(10.0, f64(f32(snr_db) / f32(20))))
    a_signal = f32(f64(spn) / (f64(spn) + 1.0))
    a_noise = f32(1.0 / (f64(spn) + 1.0))
    return a_signal, f32(f64(a_noise) * 0.707)


def awgn_mix(x, noise, a_signal, g_noise):
    """out = fl(in * a_signal) + fl(noise * g): two rounded products, one rounded sum, per part"""
    xf = np.ascontiguousarray(x, c64).view(f32)
    nf = np.ascontiguousarray(noise, c64).view(f32)
    return ((xf * f32(a_signal)).astype(f32) + (nf * f32(g_noise)).astype(f32)).astype(f32).view(c64)


def awgnfile_noise(noise_file, bufsize, n_blocks):
    """the noise of `n_blocks` blocks of awgn_cc --awgnfile: a short read rewinds and reads a whole block again, so the file's whole blocks cycle 0, 1, ..,
    0, 1, .. and its partial tail is never used"""
    noise_file = np.ascontiguousarray(noise_file, c64)
    whole = noise_file.size // bufsize
    assert whole >= 1
    return np.concatenate([noise_file[(b % whole) * bufsize:(b % whole + 1) * bufsize] for b in range(n_blocks)]) if n_blocks else np.zeros(0, c64)


def awgn_cc_file(x, snr_db, noise_file, bufsize):
    """`csdr awgn_cc snr_db --awgnfile F` on the whole blocks of x"""
    x = np.ascontiguousarray(x, c64)
    nb = x.size // bufsize
    a, g = awgn_gains(snr_db)
    return awgn_mix(x[:nb * bufsize], awgnfile_noise(noise_file, bufsize, nb), a, g)


def total_logpower_cf(x):
    x = np.asarray(x).astype(np.complex128)
    return 10 * np.log10(np.mean(x.real ** 2 + x.imag ** 2))


def normalized_timing_variance_u32_f(idx, samples_per_symbol, initial_sample_offset):
    """the reference's unsigned arithmetic, its float32 running mean and its float32 sum; one index: 0 / 0 = NaN, none: 0"""
    idx = np.asarray(idx, u32)
    n, sps, off = idx.size, u32(samples_per_symbol), u32(initial_sample_offset)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        d = (idx - off).astype(u32)
        nearest = (d // sps + (d % sps > sps // u32(2))).astype(u32)
        correct = (off + nearest * sps).astype(u32)
        sodiff = np.abs((correct - idx).astype(u32).view(np.int32))
        rad = ((sodiff.astype(f32) / f32(samples_per_symbol)).astype(f32) * f32(3.14159265358979323846)).astype(f32)
        mean = f32(0)
        for i in range(n):
            mean = f32(f32(mean * f32(f32(i) / f32(i + 1))) + f32(rad[i] / f32(i + 1)))
        result = f32(0)
        for i in range(n):
            dd = f32(rad[i] - mean)
            result = f32(result + f32(f32(dd * dd) / f32(n - 1)))
    return result
