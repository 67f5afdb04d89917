"""Float64 restatement of exact t-SNE at two components as include/bsed.h states it (``bsed_tsne_affinities``,
``bsed_tsne_gradient``, ``bsed_tsne_update``) and as bsed_amd/tsne.py drives it, in plain numpy from the SAME float32
inputs the kernels read.  Nothing here is shared with the product.  tests/test_tsne_reference_cpu.py pins it to sklearn's
own ``_joint_probabilities``, ``_kl_divergence``, ``_gradient_descent`` and ``TSNE(method="exact")``;
tests/test_tsne_gpu.py compares the kernels with it under the bounds below.

Derived bounds, first order in u = 2^-24 (the unit round-off of float32); the float64 operations of the kernels (the sums
over a row, exp, log) are allotted 1e-12 relative.  With a_j = beta d2(i,j), p_j = p(j|i) and <.> the mean under p:

A. Conditional probabilities at the beta the kernel returns.  The kernel's d2 is within (D + 3) u of the float64 one
   (tests/test_domain_gap_gpu.py, bound 1) and the beta it used is within u of the float32 value it returns, so
   exp(-d2 beta) is off by the factor exp(+-delta_j), delta_j = a_j (D + 4) u; their sum by at most the p-weighted mean
   delta_S = <delta>; the quotient is rounded to float32 once (2 u allotted, and 2^-149 for a subnormal result):
       |p_hat_j - p_j| <= p_j (expm1(delta_j + delta_S) + 2 u) + 2^-149                                 (cond_bound)
B. Entropy at that beta.  H = log S + beta SUM_j d2_j e_j / S with e_j = exp(-a_j);  dH / d log e_j = p_j (1 + a_j - <a>),
   and the explicit d2 and beta of the second term carry (D + 4) u of <a>:
       |H_64(beta_hat) - log perplexity| <= 1e-5 + SUM_j p_j |1 + a_j - <a>| delta_j + <a> (D + 4) u + 1e-12   (entropy_bound)
   (1e-5 is the float32 value sklearn's constant has.)  Two betas that both meet the stop rule -- the kernel's and the
   restatement's -- therefore have entropies within 2e-5 plus twice that round-off of each other: that is what the stop
   rule allows, and the beta test is made in terms of H, which is monotone in beta.
C. Joint affinities.  P_ij = fl32(p_hat(j|i) + p_hat(i|j)):  the two bounds of A plus u (p_j|i + p_i|j).       (joint_bound)
D. Gradient.  Per pair in float32: the difference y_i - y_j (u), |.|^2 (3 u more), 1 + . (u), the reciprocal (u): w is
   within 6 u; P w (y_i - y_j): 3 u more; w^2 (y_i - y_j): 13 u + 2 u; four columns added in float32: 3 u more.  So the
   attraction sum is within 12 u of SUM_j P w |dy|, the repulsion sum within 18 u of SUM_j w^2 |dy| and Z within 9 u
   of itself; the gradient is rounded to float32 once:
       |g_hat - g| <= 4 (s 12 u A_abs + 27 u R_abs / Z) + u |g| + 1e-12 (...) + 2^-149,  s = exaggeration / sum_p  (grad_bound)
   Z: 9 u Z.  |grad|^2: SUM (2 |g| b + b^2) over the elements, b their bound.  KL (float64 but for Z):
   9 u SUM p + 1e-11 SUM p |log(p / q)|.
E. Leaving sklearn's clamp of q out of the gradient moves an element by at most 4 * 2.2e-16 * SUM_j w |dy|  (clamp_bound).
"""
import numpy as np

from d2_reference import U, d2_matrix  # noqa: F401  (the tests read them as R.U and R.d2_matrix)

EPS = float(np.finfo(np.float64).eps)
TOL = float(np.float32(1e-5))                           # sklearn's PERPLEXITY_TOLERANCE is a C float
TINY_SUM = float(np.float32(1e-8))                      # and so is its EPSILON_DBL
STEPS = 100
TINY = 2.0 ** -149


def row_entropy(d, beta):
    """the N - 1 squared distances of one row, beta -> (sum, H, e) as the search evaluates them"""
    e = np.exp(-d * beta)
    s = e.sum()
    if s == 0.0:
        s = TINY_SUM
    return s, np.log(s) + beta * (d * e).sum() / s, e


def search(d2, perplexity):
    """(N, N) squared distances -> (beta (N) = the last beta evaluated per row, steps (N) = evaluations made): sklearn's
    ``_binary_search_perplexity`` rule for rule, one row after the other"""
    N = d2.shape[0]
    target = np.log(float(np.float32(perplexity)))
    betas, steps = np.empty(N), np.empty(N, np.int64)
    for i in range(N):
        d = np.delete(d2[i], i)
        beta, lo, hi = 1.0, -np.inf, np.inf
        for step in range(STEPS):
            used = beta
            diff = row_entropy(d, beta)[1] - target
            if abs(diff) <= TOL:
                break
            if diff > 0.0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
        betas[i], steps[i] = used, step + 1
    return betas, steps


def conditional(d2, beta):
    """-> (cond (N, N) with a zero diagonal: row i = p(.|i) at beta[i], H (N) the entropies)"""
    N = d2.shape[0]
    cond, H = np.zeros((N, N)), np.empty(N)
    for i in range(N):
        keep = np.arange(N) != i
        s, H[i], e = row_entropy(d2[i, keep], float(beta[i]))
        cond[i, keep] = e / s
    return cond, H


def joint(cond):
    """-> (P = cond + cond.T, NOT normalised; its sum)"""
    P = cond + cond.T
    return P, float(P.sum())


def affinities(x, perplexity):
    d2 = d2_matrix(x)
    beta, steps = search(d2, perplexity)
    cond, H = conditional(d2, beta)
    P, sum_p = joint(cond)
    return dict(d2=d2, beta=beta, steps=steps, cond=cond, H=H, P=P, sum_p=sum_p)


def gradient(y, P, inv_sum_p, exaggeration=1.0, clamp_q=False):
    """y (N, 2) float32, P (N, N) unnormalised -> dict: grad (N, 2) float64, Z, kl, and what the bounds are made of.
    ``clamp_q``: with sklearn's max(q, eps) inside the gradient (what the kernel leaves out)"""
    y32 = np.asarray(y, np.float32)
    y = y32.astype(np.float64)
    N = y.shape[0]
    exact = y[:, None, :] - y[None, :, :]
    w = 1.0 / (1.0 + (exact ** 2).sum(-1))
    # the direction y_i - y_j is the float32 difference, as in sklearn (``X_embedded[i] - X_embedded`` on its float32
    # map) and in the kernel; the distances inside w are exact, as scipy's pdist makes them
    diff = (y32[:, None, :] - y32[None, :, :]).astype(np.float64)
    np.fill_diagonal(w, 0.0)
    Z = float(w.sum())
    s = float(exaggeration) * float(inv_sum_p)
    p = s * np.asarray(P, np.float64)
    q = w / Z
    qg = np.maximum(q, EPS) if clamp_q else q
    coef = (p - qg) * w
    np.fill_diagonal(coef, 0.0)
    grad = 4.0 * (coef[:, :, None] * diff).sum(1)
    off = ~np.eye(N, dtype=bool)
    ratio = np.maximum(p[off], EPS) / np.maximum(q[off], EPS)
    terms = p[off] * np.log(ratio)
    a_abs = (np.asarray(P, np.float64) * w)[:, :, None] * np.abs(diff)
    r_abs = (w * w)[:, :, None] * np.abs(diff)
    return dict(grad=grad, Z=Z, kl=float(terms.sum()), a_abs=a_abs.sum(1), r_abs=r_abs.sum(1),
                w_abs=(w[:, :, None] * np.abs(diff)).sum(1), p_sum=float(p[off].sum()),
                kl_abs=float(np.abs(terms).sum()), s=s, mag=4.0 * (s * a_abs.sum(1) + r_abs.sum(1) / Z))


def update_step(y, grad, update, gains, momentum, learning_rate, min_gain=0.01):
    """sklearn's step in float32, every operation rounded on its own -> (y, update, gains), new arrays"""
    y, grad, update, gains = (np.asarray(a, np.float32) for a in (y, grad, update, gains))
    m, lr, mg = np.float32(momentum), np.float32(learning_rate), np.float32(min_gain)
    inc = update * grad < np.float32(0.0)
    gains = np.where(inc, gains + np.float32(0.2), gains * np.float32(0.8)).astype(np.float32)
    gains = np.where(gains < mg, mg, gains).astype(np.float32)
    scaled = (grad * gains).astype(np.float32)
    update = ((m * update).astype(np.float32) - (lr * scaled).astype(np.float32)).astype(np.float32)
    return (y + update).astype(np.float32), update, gains


def pca_init(x):
    """the two leading principal component scores by an SVD in float64, first column scaled to a standard deviation of
    1e-4, each column's entry of largest magnitude positive -> (N, 2) float32"""
    x = np.asarray(x, np.float64)
    c = x - x.mean(axis=0)
    u, s, _ = np.linalg.svd(c, full_matrices=False)
    k = min(2, s.shape[0])
    y = u[:, :k] * s[:k]
    y = y * np.where(y[np.abs(y).argmax(axis=0), np.arange(k)] < 0, -1.0, 1.0)
    if k < 2:
        y = np.concatenate([y, np.zeros((x.shape[0], 2 - k))], axis=1)
    return (y / y[:, 0].std() * 1e-4).astype(np.float32)


def auto_learning_rate(n, early_exaggeration=12.0):
    return max(n / early_exaggeration / 4.0, 50.0)


def run(P, sum_p, y0, learning_rate, max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7,
        early_exaggeration=12.0, trace=None):
    """the driver: sklearn's two phases on a float32 map with the float64 gradient rounded to float32 -> dict: y,
    kl_last (the error of the last evaluation, made before the last step: sklearn's kl_divergence_), n_iter, kl (of the
    returned map).  ``trace``: a list that receives (i, y, grad, update, gains, exaggeration, momentum) BEFORE each step"""
    y = np.asarray(y0, np.float32).copy()
    inv = 1.0 / sum_p
    error, it = np.finfo(float).max, 0

    def descend(it, last, momentum, exaggeration, patience):
        nonlocal y
        update, gains = np.zeros_like(y), np.ones_like(y)
        error = best_error = np.finfo(float).max
        best_iter = i = it
        for i in range(it, last):
            check = (i + 1) % 50 == 0
            g = gradient(y, P, inv, exaggeration)
            grad = g["grad"].astype(np.float32)
            if check or i == last - 1:
                error = g["kl"]
            if trace is not None:
                trace.append((i, y.copy(), grad.copy(), update.copy(), gains.copy(), exaggeration, momentum))
            y, update, gains = update_step(y, grad, update, gains, momentum, learning_rate)
            if check:
                norm = float(np.linalg.norm((grad * gains).astype(np.float64)))
                if error < best_error:
                    best_error, best_iter = error, i
                elif i - best_iter > patience:
                    break
                if norm <= min_grad_norm:
                    break
        return error, i

    error, it = descend(0, 250, 0.5, float(early_exaggeration), 250)
    if it < 249 or max_iter > 250:
        error, it = descend(it + 1, max_iter, 0.8, 1.0, n_iter_without_progress)
    return dict(y=y, kl_last=float(error), n_iter=it, kl=gradient(y, P, inv, 1.0)["kl"])


def kl_of_map(x, y, perplexity):
    """the float64 KL divergence of a map y of the points x"""
    a = affinities(x, perplexity)
    return gradient(y, a["P"], 1.0 / a["sum_p"], 1.0)["kl"]


def nn_accuracy(y, labels):
    """the leave-one-out 1-NN accuracy of the labels in the map"""
    d = d2_matrix(y)
    np.fill_diagonal(d, np.inf)
    labels = np.asarray(labels)
    return float((labels[d.argmin(axis=1)] == labels).mean())


# ---- the derived bounds (the module's header) ----
def _row_terms(d2, beta, i, D):
    keep = np.arange(d2.shape[0]) != i
    d = d2[i, keep]
    a = d * beta
    s, _, e = row_entropy(d, beta)
    p = e / s
    delta = a * (D + 4) * U
    return keep, a, p, delta


def cond_bound(d2, beta, D):
    """(N, N) bound A on the conditional probabilities at ``beta``"""
    N = d2.shape[0]
    out = np.zeros((N, N))
    for i in range(N):
        keep, a, p, delta = _row_terms(d2, float(beta[i]), i, D)
        out[i, keep] = p * (np.expm1(delta + (p * delta).sum()) + 2 * U) + TINY
    return out


def entropy_bound(d2, beta, D):
    """(N) the round-off part of bound B (without the 1e-5 of the stop rule)"""
    N = d2.shape[0]
    out = np.empty(N)
    for i in range(N):
        _, a, p, delta = _row_terms(d2, float(beta[i]), i, D)
        mean_a = (p * a).sum()
        out[i] = (p * np.abs(1.0 + a - mean_a) * delta).sum() + mean_a * (D + 4) * U + 1e-12
    return out


def joint_bound(cond, cb):
    return cb + cb.T + U * (cond + cond.T)


def grad_bound(g):
    """(N, 2) bound D on the gradient elements, from ``gradient``'s dict"""
    return (4.0 * (g["s"] * 12 * U * g["a_abs"] + 27 * U * g["r_abs"] / g["Z"]) + U * np.abs(g["grad"])
            + 1e-12 * g["mag"] + TINY)


def clamp_bound(g):
    return 4.0 * EPS * g["w_abs"]
