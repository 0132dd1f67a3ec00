"""Host-side evaluation of H = prod_s B_s / A_s on the rFFT grid and of its coefficient gradients in extended precision (np.longdouble,
64-bit significand on x86-64): the yardstick the fft_freqz tests measure BOTH the device kernel and the reference's float64 golden
responses against. The reference's float64 H comes from zero-padded FFTs; for a pole close to the unit circle (a 20 Hz shelf, a high-Q
band near Nyquist) those carry up to ~5e-11 relative error in H and ~3e-10 in the gradients, so a fixed tolerance against the golden
alone would measure the golden, not the kernel."""
import numpy as np


def exact_response(b, a, n_fft, W=None):
    """b (rows, S, Kb), a (rows, S, Ka) real -> H (rows, n_fft // 2 + 1) complex128 and, with a cotangent W (rows, bins), the
    gradients of sum(Re(conj(W) H)) w.r.t. b and a (float64, like b and a); taps j >= n_fft are cropped as rfft crops them."""
    ld = np.longdouble
    n = int(n_fft)
    k = np.arange(n // 2 + 1)
    # the angle -pi (2k mod 2n) / n with pi and the division in long double (the reduction is exact in integers, as in the kernel)
    pi = 4 * np.arctan(ld(1))
    ang = -pi * ((2 * k) % (2 * n)).astype(ld) / ld(n)
    z = np.empty(k.shape, np.clongdouble)
    z.real, z.imag = np.cos(ang), np.sin(ang)
    rows, S, Kb0 = b.shape
    Ka0 = a.shape[2]
    Kb, Ka = min(Kb0, n), min(Ka0, n)

    def poly(c):
        acc = np.zeros((rows, z.size), np.clongdouble) + c[:, -1:].astype(ld)
        for j in range(c.shape[1] - 2, -1, -1):
            acc = acc * z + c[:, j:j + 1].astype(ld)
        return acc

    B = [poly(b[:, s, :Kb]) for s in range(S)]
    A = [poly(a[:, s, :Ka]) for s in range(S)]
    N, D = np.prod(B, 0), np.prod(A, 0)
    H = N / D
    if W is None:
        return H.astype(np.complex128)
    W = np.asarray(W).astype(np.clongdouble)
    gb, ga = np.zeros(b.shape, ld), np.zeros(a.shape, ld)
    zc = np.conj(z)
    for s in range(S):
        excl = np.prod([B[t] for t in range(S) if t != s], 0) if S > 1 else np.ones_like(N)
        u = np.conj(excl / D) * W
        v = -np.conj(H / A[s]) * W
        w = np.ones_like(z)
        for j in range(max(Kb, Ka)):
            if j < Kb:
                gb[:, s, j] = np.real(w * u).sum(-1)
            if j < Ka:
                ga[:, s, j] = np.real(w * v).sum(-1)
            w = w * zc
    return H.astype(np.complex128), gb.astype(np.float64), ga.astype(np.float64)


def exact_for_golden(g):
    """(H, [gradients in the golden's layout]) for one golden file (tests/golden/freqz_*.npz)."""
    n = int(g["n_fft"])
    if "sos" in g:
        s = g["sos"].astype(np.float64)
        H, gb, ga = exact_response(s[..., :3], s[..., 3:], n, g["W"])
        return H, [np.concatenate([gb, ga], -1)]
    b, a = g["b"].astype(np.float64), g["a"].astype(np.float64)
    lead = np.broadcast_shapes(b.shape[:-1], a.shape[:-1])
    bb = np.broadcast_to(b, lead + b.shape[-1:]).reshape(-1, 1, b.shape[-1])
    aa = np.broadcast_to(a, lead + a.shape[-1:]).reshape(-1, 1, a.shape[-1])
    H, gb, ga = exact_response(bb, aa, n, g["W"].reshape(-1, g["W"].shape[-1]))
    gb = gb.reshape(lead + b.shape[-1:])
    ga = ga.reshape(lead + a.shape[-1:])
    # gradients of broadcast inputs: summed over the broadcast dimensions
    def reduce(gr, shape):
        while gr.ndim > len(shape):
            gr = gr.sum(0)
        for i, d in enumerate(shape):
            if d == 1 and gr.shape[i] != 1:
                gr = gr.sum(i, keepdims=True)
        return gr
    return H.reshape(lead + (H.shape[-1],)), [reduce(gb, b.shape), reduce(ga, a.shape)]


def fp64_bound(g):
    """Per bin, an a-priori bound on the error of ANY float64 evaluation of H from the golden's coefficients: Horner's rule in float64
    errs by at most gamma_2K sum_j |c_j| per polynomial (gamma_m = m u / (1 - m u), u = 2^-53), and a twiddle z rounded by 2 u moves
    each polynomial by at most 2 u sum_j j |c_j|; propagated through H = prod B_s / prod A_s to first order:
        |dH| <= sum_s [ e(b_s) |prod_{t != s} B_t| / |D| + e(a_s) |H| / |A_s| ],  e(c) = sum_j (gamma_2K + 2 u j) |c_j|.
    Next to a pole on the unit circle |A_s| is the small difference of O(1) terms and this bound, not 1e-12, is the floor."""
    u = 2.0 ** -53
    n = int(g["n_fft"])
    if "sos" in g:
        s = g["sos"].astype(np.float64)
        b, a = s[..., :3], s[..., 3:]
    else:
        b0, a0 = g["b"].astype(np.float64), g["a"].astype(np.float64)
        lead = np.broadcast_shapes(b0.shape[:-1], a0.shape[:-1])
        b = np.broadcast_to(b0, lead + b0.shape[-1:]).reshape(-1, 1, b0.shape[-1])
        a = np.broadcast_to(a0, lead + a0.shape[-1:]).reshape(-1, 1, a0.shape[-1])
    b, a = b[..., :n], a[..., :n]
    rows, S = b.shape[:2]
    z = np.exp(-2j * np.pi * np.arange(n // 2 + 1) / n)

    def ev(c):
        return np.stack([np.polynomial.polynomial.polyval(z, c[:, s].T) for s in range(S)], 1)      # (rows, S, bins)

    def e(c):
        K = c.shape[-1]
        gam = 2 * K * u / (1 - 2 * K * u)
        return ((gam + 2 * u * np.arange(K)) * np.abs(c)).sum(-1)[..., None]                          # (rows, S, 1)

    B, A = ev(b), ev(a)
    D = np.prod(A, 1)
    H = np.prod(B, 1) / D
    bound = np.zeros(H.shape)
    for s in range(S):
        excl = np.prod(np.delete(B, s, 1), 1) if S > 1 else np.ones_like(H)
        bound += e(b)[:, s] * np.abs(excl) / np.abs(D) + e(a)[:, s] * np.abs(H) / np.abs(A[:, s])
    return bound
