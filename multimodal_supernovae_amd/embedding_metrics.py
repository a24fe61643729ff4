"""What the contrastive embedding itself looks like: alignment and uniformity (Wang & Isola 2020), the modality gap (Liang et
al. 2022), effective rank / RankMe (Garrido et al. 2023), and recall@k, MRR and median rank in both directions.

    pair_potential, pair_alignment
                      the two pair sums in fp64 on the device (csrc/embedding_metrics.hip: msn_pair_potential sums
                      exp(-t d^2) and d^2 over all pairs without writing the N x N matrix; msn_pair_alignment sums d^2 and d
                      over partner rows).  Enqueue only.
    pair_field        per row r_i = sum_j exp(-t d^2_ij) and F_i = sum_j exp(-t d^2_ij) (x_i - y_j) in fp64 on the device
                      (csrc/uniformity_loss.hip: msn_pair_field, a second fp64 matrix product behind the scores): what the
                      gradient of the uniformity needs (loss.align_uniform_loss).  D <= 256.  Enqueue only.
    column_covariance the column means and the covariance of the centred rows in fp64 on the device (csrc/vicreg.hip:
                      msn_column_cov): what loss.vicreg_loss regularises.  D <= 256.  Enqueue only.  (covariance_spectrum still
                      goes through probes.probe_gram.)  column_covariance_reference is its longdouble restatement.
    cross_correlation the column means, the biased variances, the cross covariance and the cross correlation of two towers in
                      fp64 on the device (csrc/barlow.hip: msn_cross_cov, msn_barlow_fwd): what loss.barlow_twins_loss drives to
                      the identity.  D <= 256.  Enqueue only.  cross_correlation_reference is its longdouble restatement.
    hsic_sums         the sixteen sums centred kernel alignment is made of, in fp64 on the device, for two sets whose widths may
                      differ (csrc/cka.hip: msn_hsic_sums carries a Gram tile of X and one of Y at once and never writes an
                      N x N matrix): linear or RBF kernel, with and without the diagonal.  D <= 1024.  Enqueue only.
    hsic_from_sums, cka_from_sums
                      host halves: biased HSIC (tr(KHLH) / (n - 1)^2) or the debiased estimator of Song et al. 2012 from the
                      sums, and CKA = HSIC(K, L) / sqrt(HSIC(K, K) HSIC(L, L)) (Kornblith et al. 2019); no GPU needed
    cka, cka_matrix   the figure of one call, and the layers-by-layers matrix of two lists of sets: one host copy each
    CKA               reset / update(X, Y) / compute(): minibatch CKA (Nguyen et al. 2021), debiased by default
    hsic_sums_reference, hsic_reference, cka_reference
                      numpy longdouble restatements over explicit N x N matrices; hsic_reference and cka_reference take the
                      matrix definitions and do not go through the sums
    uniformity, cross_uniformity, alignment
                      the figures of one call: one host copy each
    covariance_spectrum, effective_rank, participation_ratio, modality_gap
                      host halves over probes.probe_gram's matrix, numpy fp64: importable and testable without a GPU
    recall_at_k, mean_reciprocal_rank, median_rank, retrieval_metrics
                      over the integer ranks of utils.retrieval_ranks
    EmbeddingMetrics  reset / update(e1, e2) / compute() over a validation epoch; cka=True adds linear CKA, biased and debiased
    pair_potential_reference, pair_alignment_reference, pair_field_reference
                      numpy longdouble restatements of the kernels, importable without a GPU

No scipy or scikit-learn at run time.  Nothing here issues a collective: with several ranks, gather the embeddings before the
call, as for a kNN probe.  Not built: collectives, sample weights, D > 1024; of the alignment + uniformity loss
(loss.align_uniform_loss): D > 256, global negatives across ranks, alpha other than 1 and 2; of CKA: a median-heuristic
bandwidth (the derived one is the mean squared distance), kernels other than linear and RBF, CKA as a training loss, and sharing
HSIC(K, K) across the cells of cka_matrix.
"""
import numpy as np
import torch

from . import _lib
from ._device_args import ld, rows_on_gpu, workspace
from ._lib import check, lib, ptr, stream_ptr

MAX_D = 1024
_MODES = {"all": 0, "offdiag": 1, "within": 2}


# ------------------------------------------------------------------------------------------------- host: the spectrum
def _gram_parts(G, D, who):
    G = np.asarray(G, dtype=np.float64)
    D = int(D)
    if D < 1 or G.ndim != 2 or G.shape[0] != G.shape[1] or G.shape[0] < D + 1:
        raise ValueError(f"{who}: G must be a probe_gram matrix of at least ({D + 1}, {D + 1}) for D = {D} (got {G.shape})")
    n = G[D, D]
    if n < 1:
        raise ValueError(f"{who}: the Gram matrix holds no rows")
    return G[:D, :D], G[:D, D], n


def covariance_spectrum(G, D, center=True):
    """Singular values, descending, of the centred (N, D) embedding matrix -- with center=False of the matrix itself -- from
    probes.probe_gram's G: sqrt(max(lambda, 0)) over eigvalsh(X^T X - s s^T / n), s the column sums.  What a Gram matrix costs:
    a singular value below sqrt(2^-52) of the largest is noise (the tests measure 1.3e-6 on rank-3 data)."""
    A, s, n = _gram_parts(G, D, "covariance_spectrum")
    if center:
        A = A - np.outer(s, s) / n
    lam = np.linalg.eigvalsh((A + A.T) / 2)
    return np.sqrt(np.maximum(lam, 0.0))[::-1].copy()


def effective_rank(s, eps=1e-7):
    """exp(-sum p log p) with p = s / sum s + eps over singular values s: RankMe (Garrido et al. 2023) for the spectrum of the
    uncentred matrix (covariance_spectrum(..., center=False))."""
    s = np.asarray(s, dtype=np.float64)
    p = s / s.sum() + eps
    return float(np.exp(-np.sum(p * np.log(p))))


def participation_ratio(s):
    """(sum s^2)^2 / sum s^4 over singular values s: the participation ratio of the covariance eigenvalues s^2."""
    s2 = np.asarray(s, dtype=np.float64) ** 2
    return float(s2.sum() ** 2 / np.sum(s2 ** 2))


def modality_gap(Gx, Gy, D):
    """|mean(X) - mean(Y)|_2 (Liang et al. 2022) from the column sums of the two sets' probe_gram matrices."""
    _, sx, nx = _gram_parts(Gx, D, "modality_gap")
    _, sy, ny = _gram_parts(Gy, D, "modality_gap")
    return float(np.linalg.norm(sx / nx - sy / ny))


# ---------------------------------------------------------------------------------------------------- host: retrieval
def _ranks(ranks, who):
    r = np.asarray(ranks.detach().cpu() if isinstance(ranks, torch.Tensor) else ranks)
    if r.ndim != 1 or len(r) == 0 or not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f"{who}: ranks must be a non-empty vector of integers (got {r.dtype} {r.shape})")
    return r.astype(np.int64)


def recall_at_k(ranks, k):
    """Share of the rows whose partner is among the k most similar: rank < k, rank = the number of rows strictly more similar
    than the partner (utils.retrieval_ranks)."""
    if int(k) < 1:
        raise ValueError(f"recall_at_k: k must be at least 1 (got {k})")
    r = _ranks(ranks, "recall_at_k")
    return float(np.count_nonzero(r < int(k)) / len(r))


def mean_reciprocal_rank(ranks):
    """Mean of 1 / (rank + 1)."""
    return float(np.mean(1.0 / (_ranks(ranks, "mean_reciprocal_rank") + 1.0)))


def median_rank(ranks):
    """Median of the 1-based ranks rank + 1 (the mean of the two middle values for an even count)."""
    return float(np.median(_ranks(ranks, "median_rank") + 1))


def _top_k(top_k):
    ks = tuple(int(k) for k in top_k)
    if not ks or min(ks) < 1:
        raise ValueError(f"top_k must name at least one k >= 1 (got {top_k!r})")
    return ks


def _retrieval_from_ranks(r_a2b, r_b2a, ks):
    out = {}
    for sfx, r in (("_a2b", r_a2b), ("_b2a", r_b2a)):
        for k in ks:
            out[f"recall{k}{sfx}"] = recall_at_k(r, k)
        out[f"mrr{sfx}"] = mean_reciprocal_rank(r)
        out[f"medr{sfx}"] = median_rank(r)
    for key in [f"recall{k}" for k in ks] + ["mrr", "medr"]:
        out[key] = 0.5 * (out[key + "_a2b"] + out[key + "_b2a"])
    return out


def retrieval_metrics(e1, e2, top_k=(1, 5, 10)):
    """recall{k}, mrr and medr of a CLIP-style retrieval over (N, D) partner sets, by cosine similarity: `_a2b` queries with
    the rows of e1 and ranks the rows of e2 (utils.retrieval_ranks(e2, e1)), `_b2a` the other way round; the keys without a
    suffix are the means of the two directions.  Two host copies of N ints."""
    from .utils import retrieval_ranks
    ks = _top_k(top_k)
    return _retrieval_from_ranks(retrieval_ranks(e2, e1).cpu().numpy(), retrieval_ranks(e1, e2).cpu().numpy(), ks)


# -------------------------------------------------------------------------------------------- host: the kernels restated
def pair_potential_reference(X, Y=None, t=2.0, pairs="within"):
    """numpy longdouble restatement of msn_pair_potential: (sum exp(-t d2), sum d2) over the pair set, d2 in the direct form
    sum_c (x_c - y_c)^2."""
    if pairs not in _MODES:
        raise ValueError(f"pair_potential_reference: pairs must be 'within', 'all' or 'offdiag' (got {pairs!r})")
    X = np.asarray(X, dtype=np.float32).astype(np.longdouble)
    Y = X if Y is None else np.asarray(Y, dtype=np.float32).astype(np.longdouble)
    if pairs == "within" and Y is not X:
        raise ValueError("pair_potential_reference: 'within' pairs the rows of X with each other")
    if X.ndim != 2 or Y.ndim != 2 or X.shape[1] != Y.shape[1] or (pairs == "offdiag" and len(X) != len(Y)):
        raise ValueError(f"pair_potential_reference: X (Nx, D) and Y (Ny, D) needed (got {X.shape} and {Y.shape})")
    t = np.longdouble(t)
    se = sd = np.longdouble(0)
    for i, x in enumerate(X):
        d2 = ((Y - x) ** 2).sum(axis=1)
        if pairs == "within":
            d2 = d2[i + 1:]
        elif pairs == "offdiag":
            d2 = np.delete(d2, i)
        se += np.exp(-t * d2).sum()
        sd += d2.sum()
    return se, sd


def pair_alignment_reference(X, Y):
    """numpy longdouble restatement of msn_pair_alignment: (sum d2, sum sqrt(d2), d2 per row)."""
    X = np.asarray(X, dtype=np.float32).astype(np.longdouble)
    Y = np.asarray(Y, dtype=np.float32).astype(np.longdouble)
    if X.ndim != 2 or X.shape != Y.shape:
        raise ValueError(f"pair_alignment_reference: two (N, D) sets of equal shape needed (got {X.shape} and {Y.shape})")
    d2 = ((X - Y) ** 2).sum(axis=1)
    return d2.sum(), np.sqrt(d2).sum(), d2


def _self_offset(exclude_self, self_offset):
    off = (0 if exclude_self else -1) if self_offset is None else int(self_offset)
    if off < -1:
        raise ValueError(f"pair_field: self_offset must be -1 (no pair left out) or >= 0 (got {off})")
    return off


def pair_field_reference(X, Y=None, t=2.0, exclude_self=True, self_offset=None):
    """numpy longdouble restatement of msn_pair_field in the direct form: r_i = sum_j w_ij and F_i = sum_j w_ij (x_i - y_j),
    w_ij = exp(-t sum_c (x_ic - y_jc)^2), over the rows j of Y (X itself when None) but j == i + self_offset.  -> (r (Nx),
    F (Nx, D))."""
    X = np.asarray(X, dtype=np.float32).astype(np.longdouble)
    Y = X if Y is None else np.asarray(Y, dtype=np.float32).astype(np.longdouble)
    if X.ndim != 2 or Y.ndim != 2 or X.shape[1] != Y.shape[1]:
        raise ValueError(f"pair_field_reference: X (Nx, D) and Y (Ny, D) needed (got {X.shape} and {Y.shape})")
    off = _self_offset(exclude_self, self_offset)
    t = np.longdouble(t)
    r = np.zeros(len(X), dtype=np.longdouble)
    F = np.zeros(X.shape, dtype=np.longdouble)
    for i, x in enumerate(X):
        diff = x - Y
        w = np.exp(-t * (diff ** 2).sum(axis=1))
        if off >= 0 and i + off < len(Y):
            w[i + off] = 0
        r[i] = w.sum()
        F[i] = (w[:, None] * diff).sum(axis=0)
    return r, F


# ------------------------------------------------------------------------------------------------------ device halves
def _out2(out, device, who):
    if out is None:
        return torch.empty(2, dtype=torch.float64, device=device)
    if out.shape != (2,) or out.dtype != torch.float64 or out.device != device or not out.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous float64 (2,) tensor on {device}")
    return out


def pair_potential(X, Y=None, t=2.0, pairs="within", out=None):
    """out (2 doubles on the device) = (sum exp(-t d2_ij), sum d2_ij) over the pairs of rows of X (Nx, D) and Y (Ny, D):
    "within" the unordered pairs i < j of X (Y = None), "all" every (i, j), "offdiag" every (i, j) but i == j (Nx == Ny).
    d2 = max(0, |x|^2 + |y|^2 - 2 x.y) in fp64 (msn_pair_potential).  Enqueue only."""
    if pairs not in _MODES:
        raise ValueError(f"pair_potential: pairs must be 'within', 'all' or 'offdiag' (got {pairs!r})")
    X = rows_on_gpu(X, "pair_potential", "embeddings")
    if pairs == "within":
        if Y is not None:
            raise ValueError("pair_potential: 'within' pairs the rows of X with each other; pass no Y")
        Ny = 0
    else:
        if Y is None:
            raise ValueError(f"pair_potential: pairs={pairs!r} needs Y")
        Y = rows_on_gpu(Y, "pair_potential", "embeddings")
        if Y.device != X.device:
            raise _lib.MsnHipError("pair_potential: X and Y must live on the same GPU")
        if Y.shape[1] != X.shape[1]:
            raise ValueError(f"pair_potential: X has {X.shape[1]} columns, Y {Y.shape[1]}")
        Ny = Y.shape[0]
    Nx, D = X.shape
    out = _out2(out, X.device, "pair_potential")
    L = lib()
    mode = _MODES[pairs]
    ws = workspace(L.msn_pair_potential_workspace_bytes(Nx, Ny, D, mode), X.device)
    check(L.msn_pair_potential(ptr(X), ld(X), Nx, ptr(Y), ld(Y) if Y is not None else 0, Ny, D, float(t), mode, ptr(out),
                               ptr(ws), ws.numel(), stream_ptr()), "msn_pair_potential")
    return out


def pair_alignment(X, Y, out=None, rows=False):
    """out (2 doubles on the device) = (sum_i d2_i, sum_i sqrt(d2_i)) with d2_i = sum_c (x_ic - y_ic)^2 over partner rows
    (msn_pair_alignment); with rows=True returns (out, d2 (N) fp64).  Enqueue only."""
    X = rows_on_gpu(X, "pair_alignment", "embeddings")
    Y = rows_on_gpu(Y, "pair_alignment", "embeddings")
    if Y.device != X.device:
        raise _lib.MsnHipError("pair_alignment: X and Y must live on the same GPU")
    if X.shape != Y.shape:
        raise ValueError(f"pair_alignment: two (N, D) sets of equal shape needed (got {tuple(X.shape)} and {tuple(Y.shape)})")
    N, D = X.shape
    out = _out2(out, X.device, "pair_alignment")
    d2 = torch.empty(N, dtype=torch.float64, device=X.device) if rows else None
    L = lib()
    ws = workspace(L.msn_pair_alignment_workspace_bytes(N, D), X.device)
    check(L.msn_pair_alignment(ptr(X), ld(X), ptr(Y), ld(Y), N, D, ptr(out), ptr(d2), ptr(ws), ws.numel(), stream_ptr()),
          "msn_pair_alignment")
    return (out, d2) if rows else out


def pair_field(X, Y=None, t=2.0, exclude_self=True, *, self_offset=None, out=None):
    """(r (Nx) fp64, F (Nx, D) fp64) on the device: r_i = sum_j w_ij and F_i = r_i x_i - sum_j w_ij y_j = sum_j w_ij (x_i - y_j)
    with w_ij = exp(-t d2_ij) over the rows j of Y (X itself when None), d2 as pair_potential forms it (msn_pair_field).
    exclude_self leaves the pair (i, i) out; self_offset, where given, overrides it: the pair (i, i + self_offset), -1 for none.
    out: (r, F) to write into; rows of F past Nx are left alone.  D <= 256.  Enqueue only."""
    X = rows_on_gpu(X, "pair_field", "embeddings")
    Y = X if Y is None else rows_on_gpu(Y, "pair_field", "embeddings")
    if Y.device != X.device:
        raise _lib.MsnHipError("pair_field: X and Y must live on the same GPU")
    if Y.shape[1] != X.shape[1]:
        raise ValueError(f"pair_field: X has {X.shape[1]} columns, Y {Y.shape[1]}")
    off = _self_offset(exclude_self, self_offset)
    (Nx, D), Ny = X.shape, Y.shape[0]
    if out is None:
        r = torch.empty(Nx, dtype=torch.float64, device=X.device)
        F = torch.empty((Nx, D), dtype=torch.float64, device=X.device)
    else:
        r, F = out
        for name, a, shape in (("r", r, (Nx,)), ("F", F, (Nx, D))):
            if a.dtype != torch.float64 or a.device != X.device or not a.is_contiguous() or a.dim() != len(shape) or \
                    a.shape[0] < Nx or tuple(a.shape[1:]) != shape[1:]:
                raise ValueError(f"pair_field: out {name} must be a contiguous float64 tensor of at least {shape} on {X.device}")
    L = lib()
    ws = workspace(L.msn_pair_field_workspace_bytes(Nx, Ny, D), X.device)
    check(L.msn_pair_field(ptr(X), ld(X), Nx, ptr(Y), ld(Y), Ny, D, float(t), off, ptr(r), ptr(F), ptr(ws), ws.numel(),
                           stream_ptr()), "msn_pair_field")
    return r, F


COV_MAX_D = 256


def column_covariance_reference(X):
    """numpy longdouble restatement of column_covariance: (mean (D,), cov (D, D)) of the fp32 rows X, cov = Xc^T Xc / (N - 1)
    over the centred rows.  No GPU needed."""
    X = np.asarray(X, dtype=np.float32).astype(np.longdouble)
    if X.ndim != 2 or X.shape[0] < 2:
        raise ValueError(f"column_covariance_reference: (N, D) rows with N >= 2 needed (got {X.shape})")
    mean = X.sum(axis=0) / X.shape[0]
    Xc = X - mean
    return mean, Xc.T @ Xc / (X.shape[0] - 1)


def column_covariance(X, out=None):
    """(mean (D,) fp64, cov (D, D) fp64) on the device: the column means of the fp32 rows X and the covariance of the centred
    rows, cov = (X - mean)^T (X - mean) / (N - 1), symmetric bit for bit (msn_column_cov, csrc/vicreg.hip: the rows are centred
    on their way into the fp64 matrix product, so there is no X^T X - N mean mean^T cancellation).  N >= 2, D <= 256.
    out: (mean, cov) to write into.  Enqueue only."""
    X = rows_on_gpu(X, "column_covariance", "embeddings")
    N, D = X.shape
    if N < 2:
        raise _lib.MsnHipError(f"column_covariance: N must be at least 2 (got {N}): one row has no covariance")
    if not 1 <= D <= COV_MAX_D:
        raise _lib.MsnHipError(f"column_covariance: D must be in 1..{COV_MAX_D} (got {D}); wider embeddings are not built")
    if out is None:
        mean = torch.empty(D, dtype=torch.float64, device=X.device)
        cov = torch.empty((D, D), dtype=torch.float64, device=X.device)
    else:
        mean, cov = out
        for name, a, shape in (("mean", mean, (D,)), ("cov", cov, (D, D))):
            if a.dtype != torch.float64 or a.device != X.device or not a.is_contiguous() or tuple(a.shape) != shape:
                raise ValueError(f"column_covariance: out {name} must be a contiguous float64 tensor of shape {shape} on {X.device}")
    L = lib()
    ws = workspace(L.msn_column_cov_workspace_bytes(N, D), X.device)
    check(L.msn_column_cov(ptr(X), ld(X), N, D, ptr(mean), ptr(cov), ptr(ws), ws.numel(), stream_ptr()), "msn_column_cov")
    return mean, cov


def cross_correlation_reference(X, Y, eps=1e-5):
    """numpy longdouble restatement of cross_correlation: (mean_x, mean_y, var_x, var_y, cov, corr) of the fp32 rows X, Y, with
    BatchNorm's statistics: var and cov divide by N (column_covariance_reference divides by N - 1), corr[a][b] = cov[a][b] /
    (sqrt(var_x[a] + eps) sqrt(var_y[b] + eps)).  No GPU needed."""
    X = np.asarray(X, dtype=np.float32).astype(np.longdouble)
    Y = np.asarray(Y, dtype=np.float32).astype(np.longdouble)
    if X.ndim != 2 or X.shape[0] < 2 or X.shape != Y.shape:
        raise ValueError(f"cross_correlation_reference: two (N, D) sets of one shape with N >= 2 needed (got {X.shape}, {Y.shape})")
    n = np.longdouble(X.shape[0])
    mx, my = X.sum(axis=0) / n, Y.sum(axis=0) / n
    Xc, Yc = X - mx, Y - my
    vx, vy = (Xc * Xc).sum(axis=0) / n, (Yc * Yc).sum(axis=0) / n
    cov = Xc.T @ Yc / n
    eps = np.longdouble(eps)
    return mx, my, vx, vy, cov, cov / np.outer(np.sqrt(vx + eps), np.sqrt(vy + eps))


def _cross_cov(X, Y):
    """(mean_x, mean_y, var_x, var_y, cov) of two checked (N, D) fp32 sets on one device: msn_cross_cov into fresh tensors."""
    N, D = X.shape
    stats = torch.empty((4, D), dtype=torch.float64, device=X.device)
    cov = torch.empty((D, D), dtype=torch.float64, device=X.device)
    L = lib()
    ws = workspace(L.msn_cross_cov_workspace_bytes(N, D), X.device)
    check(L.msn_cross_cov(ptr(X), ld(X), ptr(Y), ld(Y), N, D, ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]), ptr(cov),
                          ptr(ws), ws.numel(), stream_ptr()), "msn_cross_cov")
    return stats[0], stats[1], stats[2], stats[3], cov


def _barlow_fwd(var_x, var_y, cov, N, lambd, eps):
    """(loss, comp, corr, M (2, D, D), d (2, D)) of msn_barlow_fwd from the statistics of _cross_cov."""
    D = cov.shape[0]
    dev = cov.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    comp = torch.empty(2, dtype=torch.float64, device=dev)
    corr = torch.empty((D, D), dtype=torch.float64, device=dev)
    M = torch.empty((2, D, D), dtype=torch.float64, device=dev)
    d = torch.empty((2, D), dtype=torch.float64, device=dev)
    L = lib()
    ws = workspace(L.msn_barlow_workspace_bytes(D), dev)
    check(L.msn_barlow_fwd(ptr(var_x), ptr(var_y), ptr(cov), N, D, lambd, eps, ptr(loss), ptr(comp), ptr(corr), ptr(M[0]), ptr(M[1]),
                           ptr(d[0]), ptr(d[1]), ptr(ws), ws.numel(), stream_ptr()), "msn_barlow_fwd")
    return loss, comp, corr, M, d


def cross_correlation(X, Y, eps=1e-5):
    """(mean_x (D,), mean_y (D,), var_x (D,), var_y (D,), cov (D, D), corr (D, D)), fp64 on the device, of the fp32 rows X, Y:
    the column means, the variances and the cross covariance of the centred rows, cov = (X - mean_x)^T (Y - mean_y) / N (not
    symmetric), and corr[a][b] = cov[a][b] / (sqrt(var_x[a] + eps) sqrt(var_y[b] + eps)).  These are BatchNorm's statistics:
    the variance and the covariance divide by N, where column_covariance divides by N - 1.  The rows are centred on their way
    into the fp64 matrix product (msn_cross_cov, csrc/barlow.hip), so nothing cancels.  N >= 2, D <= 256.  Enqueue only."""
    import math
    eps = float(eps)
    if not (eps > 0 and math.isfinite(eps)):
        raise ValueError(f"cross_correlation: eps must be finite and positive (got {eps})")
    X = rows_on_gpu(X, "cross_correlation", "embeddings")
    Y = rows_on_gpu(Y, "cross_correlation", "embeddings")
    if tuple(X.shape) != tuple(Y.shape) or X.device != Y.device:
        raise ValueError(f"cross_correlation: two (N, D) sets of one shape on one device needed (got {tuple(X.shape)}, {tuple(Y.shape)})")
    N, D = X.shape
    if N < 2:
        raise _lib.MsnHipError(f"cross_correlation: N must be at least 2 (got {N}): one row has no variance")
    if not 1 <= D <= COV_MAX_D:
        raise _lib.MsnHipError(f"cross_correlation: D must be in 1..{COV_MAX_D} (got {D}); wider embeddings are not built")
    mx, my, vx, vy, cov = _cross_cov(X, Y)
    corr = _barlow_fwd(vx, vy, cov, N, 0.0, eps)[2]
    return mx, my, vx, vy, cov, corr


# ------------------------------------------------------------------------------------------ centred kernel alignment
HSIC_KERNELS = {"linear": 0, "rbf": 1}
HSIC_SUMS = ("KL", "KK", "LL", "rKL", "rKK", "rLL", "sK", "sL")          # the columns of hsic_sums; row 0 without, row 1 with i == j
_HSIC_PAIRS = {"KL": (0, 3, 6, 7), "KK": (1, 4, 6, 6), "LL": (2, 5, 7, 7)}  # the product sum, the row-sum product, the two totals


def _hsic_kernel(kernel, who):
    if kernel not in HSIC_KERNELS:
        raise ValueError(f"{who}: kernel must be 'linear' or 'rbf' (got {kernel!r})")
    return HSIC_KERNELS[kernel]


def _sigma_pair(sigma, sigma_scale, who):
    """(sigma_x, sigma_y, sigma_scale) as floats, None for a bandwidth to derive."""
    pair = tuple(sigma) if isinstance(sigma, (tuple, list)) else (sigma, sigma)
    if len(pair) != 2:
        raise ValueError(f"{who}: sigma must be None, a float or a pair (got {sigma!r})")
    pair = tuple(None if v is None else float(v) for v in pair)
    for v in pair:
        if v is not None and not (v > 0 and np.isfinite(v)):
            raise ValueError(f"{who}: an explicit sigma must be finite and positive (got {v}); None derives it")
    scale = float(sigma_scale)
    if not (scale > 0 and np.isfinite(scale)):
        raise ValueError(f"{who}: sigma_scale must be finite and positive (got {sigma_scale})")
    return pair[0], pair[1], scale


def _kernel_matrix(Z, kernel, sigma, scale):
    """The n x n longdouble kernel matrix of the fp32 rows Z after centring, with its diagonal (|zc_i|^2, or exactly 1)."""
    Z = np.asarray(Z, dtype=np.float32).astype(np.longdouble)
    n = Z.shape[0]
    Zc = Z - Z.sum(axis=0) / np.longdouble(n)
    if kernel == "linear":
        return Zc @ Zc.T
    d2 = np.stack([((Zc - z) ** 2).sum(axis=1) for z in Zc])           # the direct form: nothing cancels
    np.fill_diagonal(d2, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        s2 = np.longdouble(sigma) ** 2 if sigma is not None else np.longdouble(scale) ** 2 * (d2.sum() / (np.longdouble(n) * (n - 1)))
        K = np.exp(-d2 / (2 * s2))                                     # equal rows, derived bandwidth: 0 / 0
    np.fill_diagonal(K, np.nan if np.isnan(K).any() else 1)          # a set without a bandwidth has no diagonal either
    return K


def _reference_matrices(X, Y, kernel, sigma, sigma_scale, who):
    _hsic_kernel(kernel, who)
    sx, sy, scale = _sigma_pair(sigma, sigma_scale, who)
    X, Y = np.asarray(X, dtype=np.float32), np.asarray(Y, dtype=np.float32)
    if X.ndim != 2 or Y.ndim != 2 or X.shape[0] != Y.shape[0] or X.shape[0] < 2 or X.shape[1] < 1 or Y.shape[1] < 1:
        raise ValueError(f"{who}: X (N, Dx) and Y (N, Dy) with N >= 2 needed (got {X.shape} and {Y.shape})")
    return _kernel_matrix(X, kernel, sx, scale), _kernel_matrix(Y, kernel, sy, scale)


def hsic_sums_reference(X, Y, kernel="linear", sigma=None, sigma_scale=1.0):
    """numpy longdouble restatement of hsic_sums over the explicit N x N matrices: a (2, 8) longdouble array, HSIC_SUMS by column,
    row 0 without and row 1 with the pairs i == j.  The RBF distances are the direct form sum_c (x_ic - x_jc)^2 and a derived
    bandwidth is sigma_scale^2 times their mean over i != j.  No GPU needed."""
    K, L = _reference_matrices(X, Y, kernel, sigma, sigma_scale, "hsic_sums_reference")
    K0, L0 = K.copy(), L.copy()
    np.fill_diagonal(K0, 0)
    np.fill_diagonal(L0, 0)
    out = np.empty((2, 8), dtype=np.longdouble)
    for c, (A, B) in enumerate(((K0, L0), (K, L))):
        rA, rB = A.sum(axis=1), B.sum(axis=1)
        out[c] = [(A * B).sum(), (A * A).sum(), (B * B).sum(), rA @ rB, rA @ rA, rB @ rB, rA.sum(), rB.sum()]
    return out


def _sums_array(sums, who):
    s = np.asarray(sums)
    if s.shape != (2, 8):
        raise ValueError(f"{who}: sums must be the (2, 8) block of hsic_sums (got {s.shape})")
    return s if s.dtype == np.longdouble else s.astype(np.float64)


def hsic_from_sums(sums, n, pair="KL", debiased=False):
    """HSIC of a pair of kernels ("KL", "KK" or "LL") from the (2, 8) block of hsic_sums over n rows:
        biased    (P1 - (2 / n) R1 + S1 S1' / n^2) / (n - 1)^2                                   = tr(KHLH) / (n - 1)^2
        debiased  (P0 + S0 S0' / ((n - 1)(n - 2)) - (2 / (n - 2)) R0) / (n (n - 3)), n >= 4       (Song et al. 2012)
    with P the sum of products, R the sum of row-sum products and S, S' the totals, the index the diagonal convention.  In fp64;
    a longdouble block is kept in longdouble, every rational factor formed there.  nan for a debiased n < 4."""
    if pair not in _HSIC_PAIRS:
        raise ValueError(f"hsic_from_sums: pair must be 'KL', 'KK' or 'LL' (got {pair!r})")
    s = _sums_array(sums, "hsic_from_sums")
    n = int(n)
    if n < 2:
        raise ValueError(f"hsic_from_sums: n must be at least 2 (got {n})")
    f = s.dtype.type
    ip, ir, ia, ib = _HSIC_PAIRS[pair]
    if debiased:
        if n < 4:
            return f("nan")
        P, R, A, B = s[0, ip], s[0, ir], s[0, ia], s[0, ib]
        return (P + A * B / (f(n - 1) * f(n - 2)) - f(2) / f(n - 2) * R) / (f(n) * f(n - 3))
    P, R, A, B = s[1, ip], s[1, ir], s[1, ia], s[1, ib]
    return (P - f(2) / f(n) * R + A * B / (f(n) * f(n))) / (f(n - 1) * f(n - 1))


def _cka_of(hkl, hkk, hll):
    """HSIC(K, L) / sqrt(HSIC(K, K) HSIC(L, L)) as a float; nan when a term of the denominator is not finite and positive."""
    if not (np.isfinite(hkk) and np.isfinite(hll) and hkk > 0 and hll > 0):
        return float("nan")
    return float(hkl / np.sqrt(hkk * hll))


def cka_from_sums(sums, n, debiased=False):
    """CKA = HSIC(K, L) / sqrt(HSIC(K, K) HSIC(L, L)) from the (2, 8) block of hsic_sums over n rows.  nan when a term of the
    denominator is <= 0 or not finite, and for a debiased n < 4; the debiased figure may be negative."""
    return _cka_of(*(hsic_from_sums(sums, n, pair, debiased) for pair in ("KL", "KK", "LL")))


def _matrix_hsic(K, L, debiased):
    n = K.shape[0]
    f = np.longdouble
    if not debiased:
        H = np.eye(n, dtype=f) - np.ones((n, n), dtype=f) / f(n)
        return np.trace(K @ H @ L @ H) / (f(n - 1) * f(n - 1))
    if n < 4:
        return f("nan")
    Kt, Lt = K.copy(), L.copy()
    np.fill_diagonal(Kt, 0)
    np.fill_diagonal(Lt, 0)
    one = np.ones(n, dtype=f)
    return (np.trace(Kt @ Lt) + (one @ Kt @ one) * (one @ Lt @ one) / (f(n - 1) * f(n - 2))
            - f(2) / f(n - 2) * (one @ Kt @ (Lt @ one))) / (f(n) * f(n - 3))


def hsic_reference(X, Y, kernel="linear", debiased=False, sigma=None, sigma_scale=1.0):
    """(HSIC(K, L), HSIC(K, K), HSIC(L, L)) in longdouble from the matrix definitions: tr(KHLH) / (n - 1)^2, or Song et al.'s
    tr(K~ L~) + 1'K~1 1'L~1 / ((n - 1)(n - 2)) - (2 / (n - 2)) 1'K~L~1 over n (n - 3) with the diagonals removed.  No GPU needed."""
    K, L = _reference_matrices(X, Y, kernel, sigma, sigma_scale, "hsic_reference")
    return _matrix_hsic(K, L, debiased), _matrix_hsic(K, K, debiased), _matrix_hsic(L, L, debiased)


def cka_reference(X, Y, kernel="linear", debiased=False, sigma=None, sigma_scale=1.0):
    """numpy longdouble CKA from the matrix definitions (hsic_reference), not through the sums: an independent route."""
    return _cka_of(*hsic_reference(X, Y, kernel, debiased, sigma, sigma_scale))


def hsic_sums(X, Y, kernel="linear", sigma=None, sigma_scale=1.0, out=None):
    """out (2, 8) fp64 on the device: HSIC_SUMS of the centred kernels K over X (N, Dx) and L over Y (N, Dy), rows are partners,
    row 0 over i != j and row 1 with the diagonal (msn_hsic_sums).  kernel "linear" (x_i . x_j of the centred rows) or "rbf"
    (exp(-|x_i - x_j|^2 / (2 sigma^2))); sigma a float or a pair (sigma_x, sigma_y), None for sigma^2 = sigma_scale^2 times the mean
    squared distance over i != j, formed on the device and never read here.  N >= 2, Dx, Dy <= 1024.  Enqueue only."""
    who = "hsic_sums"
    kid = _hsic_kernel(kernel, who)
    sx, sy, scale = _sigma_pair(sigma, sigma_scale, who)
    X = rows_on_gpu(X, who, "embeddings")
    Y = rows_on_gpu(Y, who, "embeddings")
    if Y.device != X.device:
        raise _lib.MsnHipError(f"{who}: X and Y must live on the same GPU")
    if X.shape[0] != Y.shape[0]:
        raise ValueError(f"{who}: X and Y must hold the same number of rows (got {X.shape[0]} and {Y.shape[0]})")
    (N, Dx), Dy = X.shape, Y.shape[1]
    if N < 2:
        raise _lib.MsnHipError(f"{who}: N must be at least 2 (got {N})")
    if not (1 <= Dx <= MAX_D and 1 <= Dy <= MAX_D):
        raise _lib.MsnHipError(f"{who}: Dx and Dy must be in 1..{MAX_D} (got {Dx} and {Dy}); wider embeddings are not built")
    if out is None:
        out = torch.empty((2, 8), dtype=torch.float64, device=X.device)
    elif out.shape != (2, 8) or out.dtype != torch.float64 or out.device != X.device or not out.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous float64 (2, 8) tensor on {X.device}")
    L = lib()
    ws = workspace(L.msn_hsic_workspace_bytes(N, Dx, Dy), X.device)
    check(L.msn_hsic_sums(ptr(X), ld(X), Dx, ptr(Y), ld(Y), Dy, N, kid, sx or 0.0, sy or 0.0, scale, ptr(out), ptr(ws), ws.numel(),
                          stream_ptr()), "msn_hsic_sums")
    return out


def cka(X, Y, kernel="linear", debiased=False, sigma=None, sigma_scale=1.0):
    """Centred kernel alignment of two sets of partner rows as a float: hsic_sums, one host copy, cka_from_sums."""
    sums = hsic_sums(X, Y, kernel, sigma, sigma_scale)
    return cka_from_sums(sums.cpu().numpy(), X.shape[0], debiased)


def cka_matrix(feats_a, feats_b, kernel="linear", debiased=False, sigma=None, sigma_scale=1.0):
    """The (len(feats_a), len(feats_b)) numpy array of cka(a, b): the layers-by-layers picture of two lists of (N, D) sets over
    the same N rows (the widths are free).  A host loop over hsic_sums into one buffer, one host copy at the end; HSIC(K, K) is
    formed again in every cell."""
    feats_a, feats_b = list(feats_a), list(feats_b)
    if not feats_a or not feats_b:
        raise ValueError("cka_matrix: two non-empty lists of (N, D) sets needed")
    N = feats_a[0].shape[0]
    buf = None
    for i, a in enumerate(feats_a):
        for j, b in enumerate(feats_b):
            if a.shape[0] != N or b.shape[0] != N:
                raise ValueError(f"cka_matrix: every set must hold the same {N} rows (got {a.shape[0]} and {b.shape[0]})")
            if buf is None:
                _lib.require_gpu()
                buf = torch.empty((len(feats_a), len(feats_b), 2, 8), dtype=torch.float64, device=getattr(a, "device", None))
            hsic_sums(a, b, kernel, sigma, sigma_scale, out=buf[i, j])
    h = buf.cpu().numpy()
    return np.array([[cka_from_sums(h[i, j], N, debiased) for j in range(len(feats_b))] for i in range(len(feats_a))])


class CKA:
    """Minibatch CKA (Nguyen et al. 2021) over an epoch: update(X, Y) enqueues hsic_sums of a batch and keeps its (2, 8) block and
    its size; compute() makes one host copy and returns

        sum_b HSIC(K_b, L_b) / sqrt(sum_b HSIC(K_b, K_b) sum_b HSIC(L_b, L_b)),

    debiased by default (the biased estimator depends on the batch size).  The widths of X and Y may differ from each other, not
    between batches.  nan by cka_from_sums' rules, and for a debiased batch of fewer than 4 rows."""

    def __init__(self, kernel="linear", debiased=True, sigma=None, sigma_scale=1.0):
        _hsic_kernel(kernel, "CKA")
        _sigma_pair(sigma, sigma_scale, "CKA")
        self.kernel, self.debiased, self.sigma, self.sigma_scale = kernel, bool(debiased), sigma, sigma_scale
        self.reset()

    def reset(self):
        self._sums, self._n, self._widths = [], [], None

    def update(self, X, Y):
        sums = hsic_sums(X, Y, self.kernel, self.sigma, self.sigma_scale)
        widths = (X.shape[1], Y.shape[1])
        if self._widths is not None and widths != self._widths:
            raise ValueError(f"CKA.update: the widths changed from {self._widths} to {widths}")
        self._widths = widths
        self._sums.append(sums)
        self._n.append(X.shape[0])
        return self

    def compute(self):
        if not self._sums:
            raise ValueError("CKA.compute: nothing added yet")
        h = torch.stack(self._sums).cpu().numpy()
        return _cka_of(*(sum(hsic_from_sums(h[b], n, pair, self.debiased) for b, n in enumerate(self._n))
                         for pair in ("KL", "KK", "LL")))


def _unit_rows(X, who):
    """L2-normalised rows (ops.l2norm_fwd, which takes D a multiple of 4: the rule of the kNN probes' cosine metric)."""
    from . import ops
    X = rows_on_gpu(X, who, "embeddings")
    if X.shape[1] % 4 or X.shape[1] > MAX_D:
        raise _lib.MsnHipError(f"{who}: normalize=True needs D a multiple of 4, at most {MAX_D} (got {X.shape[1]}); "
                               "pass unit rows and normalize=False otherwise")
    return ops.l2norm_fwd(X.contiguous())[0]


def _log_mean(value, count):
    return float(np.log(value / count)) if value > 0 else float("-inf")


def uniformity(X, t=2.0, normalize=True):
    """log of the mean of exp(-t |x_i - x_j|^2) over the N (N - 1) / 2 pairs i < j (Wang & Isola 2020): lower is more uniform."""
    X = _unit_rows(X, "uniformity") if normalize else X
    N = X.shape[0]
    return _log_mean(float(pair_potential(X, None, t, "within").cpu()[0]), N * (N - 1) / 2)


def cross_uniformity(X, Y, t=2.0, normalize=True, pairs="offdiag"):
    """The same over pairs of a row of X and a row of Y: "offdiag" leaves the partners i == j out, "all" keeps them."""
    if pairs not in ("offdiag", "all"):
        raise ValueError(f"cross_uniformity: pairs must be 'offdiag' or 'all' (got {pairs!r})")
    if normalize:
        X, Y = _unit_rows(X, "cross_uniformity"), _unit_rows(Y, "cross_uniformity")
    out = float(pair_potential(X, Y, t, pairs).cpu()[0])
    Nx, Ny = X.shape[0], Y.shape[0]
    return _log_mean(out, Nx * Ny - (Nx if pairs == "offdiag" else 0))


def alignment(X, Y, alpha=2, normalize=True):
    """Mean over partner rows of |x_i - y_i|^alpha, alpha = 2 or 1 (Wang & Isola 2020): lower is better aligned."""
    if alpha not in (1, 2):
        raise ValueError(f"alignment: alpha must be 2 or 1 (got {alpha!r})")
    if normalize:
        X, Y = _unit_rows(X, "alignment"), _unit_rows(Y, "alignment")
    out = pair_alignment(X, Y).cpu()
    return float(out[0 if alpha == 2 else 1]) / X.shape[0]


class EmbeddingMetrics:
    """The embedding figures of a validation epoch over two partner sets: update(e1, e2) adds a batch to two fp64 Gram
    matrices on the device (probes.probe_gram, accumulate=True) and keeps a reference to it; compute() concatenates, runs the
    pair kernels and the retrieval ranks, makes one host copy and returns

        n, alignment, uniformity_a, uniformity_b, uniformity (their mean), uniformity_cross (partners left out),
        modality_gap, erank_a, erank_b, erank (the smaller), and retrieval_metrics' keys;
        with cka=True also cka (linear, biased) and cka_debiased of the two sets (hsic_sums, in the same host copy).

    normalize: L2-normalise the rows first (D a multiple of 4).  center: take the spectra of the centred sets; center=False
    is RankMe.  No collective is issued: with several ranks the caller gathers the embeddings first, as for a kNN probe."""

    def __init__(self, t=2.0, top_k=(1, 5, 10), normalize=True, center=True, cka=False):
        if not (t > 0 and np.isfinite(t)):
            raise ValueError(f"EmbeddingMetrics: t must be finite and positive (got {t})")
        self.t, self.top_k = float(t), _top_k(top_k)
        self.normalize, self.center, self.cka = bool(normalize), bool(center), bool(cka)
        self.reset()

    def reset(self):
        self.gram_a = self.gram_b = None          # (D + 1)^2 fp64 on the device
        self._a, self._b = [], []

    def update(self, e1, e2):
        who = "EmbeddingMetrics.update"
        a = _unit_rows(e1, who) if self.normalize else rows_on_gpu(e1, who, "embeddings")
        b = _unit_rows(e2, who) if self.normalize else rows_on_gpu(e2, who, "embeddings")
        if a.shape != b.shape or a.device != b.device:
            raise ValueError(f"{who}: two (N, D) sets of equal shape on one GPU needed (got {tuple(a.shape)} and {tuple(b.shape)})")
        if self._a and a.shape[1] != self._a[0].shape[1]:
            raise ValueError(f"{who}: D changed from {self._a[0].shape[1]} to {a.shape[1]}")
        if a.shape[1] > MAX_D:
            raise _lib.MsnHipError(f"{who}: D <= {MAX_D} (got {a.shape[1]})")
        from .probes import probe_gram
        self.gram_a = probe_gram(a, out=self.gram_a, accumulate=self.gram_a is not None)
        self.gram_b = probe_gram(b, out=self.gram_b, accumulate=self.gram_b is not None)
        self._a.append(a)
        self._b.append(b)
        return self

    def compute(self):
        if not self._a:
            raise ValueError("EmbeddingMetrics.compute: nothing added yet")
        from .utils import retrieval_ranks
        A = self._a[0] if len(self._a) == 1 else torch.cat(self._a, dim=0)
        B = self._b[0] if len(self._b) == 1 else torch.cat(self._b, dim=0)
        N, D = A.shape
        M = (D + 1) * (D + 1)
        # one buffer, one copy: four pair results, the two Gram matrices, the two rank vectors (exact as doubles)
        buf = torch.empty(8 + 2 * M + 2 * N + (16 if self.cka else 0), dtype=torch.float64, device=A.device)
        pair_alignment(A, B, out=buf[0:2])
        if N >= 2:
            pair_potential(A, None, self.t, "within", out=buf[2:4])
            pair_potential(B, None, self.t, "within", out=buf[4:6])
            pair_potential(A, B, self.t, "offdiag", out=buf[6:8])
        else:
            buf[2:8].fill_(float("nan"))
        buf[8:8 + M].copy_(self.gram_a.reshape(-1))
        buf[8 + M:8 + 2 * M].copy_(self.gram_b.reshape(-1))
        buf[8 + 2 * M:8 + 2 * M + N].copy_(retrieval_ranks(B, A))          # a -> b
        buf[8 + 2 * M + N:8 + 2 * M + 2 * N].copy_(retrieval_ranks(A, B))  # b -> a
        if self.cka:
            if N >= 2:
                hsic_sums(A, B, out=buf[8 + 2 * M + 2 * N:].view(2, 8))
            else:
                buf[8 + 2 * M + 2 * N:].fill_(float("nan"))
        h = buf.cpu().numpy()
        Ga, Gb = h[8:8 + M].reshape(D + 1, D + 1), h[8 + M:8 + 2 * M].reshape(D + 1, D + 1)
        r_a2b, r_b2a = h[8 + 2 * M:8 + 2 * M + N].astype(np.int64), h[8 + 2 * M + N:8 + 2 * M + 2 * N].astype(np.int64)
        within, cross = N * (N - 1) / 2, N * (N - 1)
        out = {"n": N, "alignment": float(h[0]) / N}
        if N >= 2:
            out["uniformity_a"], out["uniformity_b"] = _log_mean(h[2], within), _log_mean(h[4], within)
            out["uniformity_cross"] = _log_mean(h[6], cross)
        else:
            out["uniformity_a"] = out["uniformity_b"] = out["uniformity_cross"] = float("nan")
        out["uniformity"] = 0.5 * (out["uniformity_a"] + out["uniformity_b"])
        out["modality_gap"] = modality_gap(Ga, Gb, D)
        out["erank_a"] = effective_rank(covariance_spectrum(Ga, D, self.center))
        out["erank_b"] = effective_rank(covariance_spectrum(Gb, D, self.center))
        out["erank"] = min(out["erank_a"], out["erank_b"])
        out.update(_retrieval_from_ranks(r_a2b, r_b2a, self.top_k))
        if self.cka:
            sums = h[8 + 2 * M + 2 * N:].reshape(2, 8)
            out["cka"] = cka_from_sums(sums, N, False) if N >= 2 else float("nan")
            out["cka_debiased"] = cka_from_sums(sums, N, True) if N >= 2 else float("nan")
        return out
