"""numpy restatement of the counter-based noise definition of include/maua_hip.h (maua_randn_frames_f32), written from the paper
(Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), not from the kernel:

  x[0..3] = Philox4x32-10(counter = (e / 4, frame, slot, 0), key = (seed low word, seed high word))
  u(x)    = ((x >> 9) + 0.5) * 2^-23
  element 4i, 4i+1 = r cos(2 pi u(x[1])), r sin(2 pi u(x[1])), r = sqrt(-2 ln u(x[0]));  4i+2, 4i+3 the same from (x[2], x[3]).

``noise_map(..., dtype=np.float64)`` is the reference the device output is compared with; ``dtype=np.float32`` evaluates the same formulas
in float32 and gives the float32-vs-float64 error that the tolerance of tests/test_randnoise_gpu.py is derived from."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
Z_MAX = float(np.sqrt(48.0 * np.log(2.0)))  # u >= 2^-24  ->  r <= sqrt(-2 ln 2^-24)


def philox4x32_10(counter, key):
    """counter: four uint32-valued arrays (broadcastable), key: two.  Returns the four output words as uint64 arrays < 2^32."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*counter)]
    k0, k1 = (np.uint64(int(v) & 0xFFFFFFFF) for v in key)
    m0, m1 = np.uint64(M0), np.uint64(M1)
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]  # 32 x 32 -> 64 bit products: exact in uint64
        c = [(p1 >> sh) ^ c[1] ^ k0, p1 & MASK, (p0 >> sh) ^ c[3] ^ k1, p0 & MASK]
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return c


def noise_map(seed, frame, slot, hw, dtype=np.float64):
    """The [hw] map of (seed, absolute frame, slot)."""
    quads = (hw + 3) // 4
    zero = np.zeros(quads, dtype=np.uint64)
    x = philox4x32_10((np.arange(quads, dtype=np.uint64), zero + np.uint64(frame), zero + np.uint64(slot & 0xFFFFFFFF), zero),
                      (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    ft = np.dtype(dtype).type
    u = [((w >> np.uint64(9)).astype(dtype) + ft(0.5)) * ft(2.0 ** -23) for w in x]
    out = np.empty((quads, 4), dtype=dtype)
    two_pi = ft(2.0 * np.pi)
    for j in (0, 2):
        r = np.sqrt(ft(-2.0) * np.log(u[j]))
        angle = two_pi * u[j + 1]
        out[:, j] = r * np.cos(angle)
        out[:, j + 1] = r * np.sin(angle)
    return out.reshape(-1)[:hw]


def noise_maps(seed, frame0, batch, slot, hw, dtype=np.float64):
    """[batch, hw]: the maps of frames frame0 .. frame0 + batch - 1."""
    return np.stack([noise_map(seed, frame0 + b, slot, hw, dtype) for b in range(batch)])


def moment_statistics(maps):
    """The seven conditions of the distribution checks, each in units of its standard error under N(0,1) i.i.d. (all must be <= 4), and
    max |z|.  ``maps``: [n_maps, hw] float64."""
    maps = np.asarray(maps, dtype=np.float64)
    z = maps.reshape(-1)
    n = z.size
    mean, var = z.mean(), z.var()
    c = z - mean
    skew = (c ** 3).mean() / var ** 1.5
    kurt = (c ** 4).mean() / var ** 2 - 3.0
    lag = lambda k: float((c[:-k] * c[k:]).mean() / var)  # noqa: E731
    cross = 0.0
    hw = maps.shape[1]
    for i in range(maps.shape[0]):
        for j in range(i + 1, maps.shape[0]):
            cross = max(cross, abs(float(np.corrcoef(maps[i], maps[j])[0, 1])))
    return {
        "mean": abs(mean) * np.sqrt(n),
        "var": abs(var - 1.0) * np.sqrt(n / 2.0),
        "skew": abs(skew) * np.sqrt(n / 6.0),
        "kurtosis": abs(kurt) * np.sqrt(n / 24.0),
        "lag1": abs(lag(1)) * np.sqrt(n),
        "lag4": abs(lag(4)) * np.sqrt(n),
        "cross": cross * np.sqrt(hw),
    }, float(np.abs(z).max())
