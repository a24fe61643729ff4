"""Linear probes on frozen embeddings: how good are the embeddings of a checkpoint?  (SURVEY.md section 2 rows 7 and 12:
the reference's evaluation script fits a linear model on the embeddings for redshift and for the class.)  The reference's
source is not pinned line by line here; the classes are named and parameterised as scikit-learn names things, and are
checked against numpy fp64 restatements in tests/test_probes_cpu.py and tests/test_probes_gpu.py.

    LinearRegressionProbe    least squares / ridge from ONE fp64 Gram matrix accumulated on the device, batch by batch
                             (csrc/probes.hip: msn_probe_gram); the (D + 1 + K)^2 matrix is the only thing that is copied
    LogisticRegressionProbe  multinomial logistic regression by L-BFGS on the host over a loss-and-gradient kernel on the
                             device (msn_logreg_loss_grad): per evaluation W goes up, 1 + C (D + 1) doubles come down
    solve_normal_equations, lbfgs
                             the host halves, pure numpy fp64: importable and testable without a GPU
    knn_search, KNeighborsRegressorProbe, KNeighborsClassifierProbe
                             exact k-nearest-neighbour search in fp64 on the device (csrc/knn.hip: msn_knn_search) and the
                             weighted mean / vote over the neighbours (msn_knn_predict_*); nothing is copied to the host
    knn_reference, knn_predict_reference
                             their numpy fp64 restatements, importable without a GPU

No scipy or scikit-learn at run time.  The classes issue no collective: with several ranks, all-reduce `probe.gram`
before `solve()`, and gather the embeddings before a kNN probe.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._device_args import ld, rows_on_gpu, workspace
from ._lib import check, lib, ptr, stream_ptr

MAX_D = 1024            # the widths the contrastive kernels take
MAX_K = 16
MAX_W = 16400           # C (D + 1) at most: W stays in LDS as doubles


# ----------------------------------------------------------------------------------------------- host: least squares
def solve_normal_equations(G, D, K, alpha=0.0, fit_intercept=True):
    """Least squares from the Gram matrix G = Z^T Z of Z = [X | 1 | Y] ((D + 1 + K)^2, fp64): returns
    (coef (K, D), intercept (K,)) of Y ~ X coef^T + intercept.

    With fit_intercept the problem is centred through the sums, as scikit-learn centres the data: with s = X^T 1,
    t = Y^T 1, A = X^T X - s s^T / n and B = X^T Y - s t^T / n.  alpha > 0 solves (A + alpha I) W = B by Cholesky
    (Ridge; the intercept is not penalised).  alpha = 0 takes the minimum-norm solution through eigh(A), dropping the
    eigenvalues <= 64 max(n, D) 2^-52 lambda_max: LinearRegression's answer also when N <= D or when columns repeat.

    What normal equations cost: the error of the coefficients grows with cond(A) = cond(X_c)^2, where a QR or SVD of the
    centred data would pay cond(X_c) only.  Unit-norm embeddings had cond(A) below 10 in every trial; data with
    cond(X_c) near 1e8 loses every digit here and should be fitted from the rows instead."""
    G = np.asarray(G, dtype=np.float64)
    D, K = int(D), int(K)
    if K < 1:
        raise ValueError("solve_normal_equations: K must be at least 1 (a Gram matrix without targets has nothing to fit)")
    if D < 1 or G.shape != (D + 1 + K, D + 1 + K):
        raise ValueError(f"solve_normal_equations: G must be ({D + 1 + K}, {D + 1 + K}) for D = {D}, K = {K} (got {G.shape})")
    if alpha < 0:
        raise ValueError("solve_normal_equations: alpha must not be negative")
    A, B = G[:D, :D], G[:D, D + 1:]
    s, t, n = G[:D, D], G[D, D + 1:], G[D, D]
    if n < 1:
        raise ValueError("solve_normal_equations: the Gram matrix holds no rows")
    if fit_intercept:
        A = A - np.outer(s, s) / n
        B = B - np.outer(s, t) / n
    if alpha > 0:
        L = np.linalg.cholesky(A + alpha * np.eye(D))
        W = np.linalg.solve(L.T, np.linalg.solve(L, B))
    else:
        lam, V = np.linalg.eigh((A + A.T) / 2)
        keep = lam > 64.0 * max(n, D) * 2.0 ** -52 * lam[-1]
        Vk = V[:, keep]
        W = Vk @ ((Vk.T @ B) / lam[keep][:, None])
    coef = W.T.copy()
    intercept = (t - coef @ s) / n if fit_intercept else np.zeros(K)
    return coef, intercept


# ------------------------------------------------------------------------------------------------------ host: L-BFGS
LbfgsResult = namedtuple("LbfgsResult", "x fun grad n_iter n_evals converged status")
LbfgsResult.__doc__ = """x, fun, grad at the end; status: "gtol" (max |g| <= gtol), "precision" (the line search found no
decrease: converged to the precision of the function) or "max_iter"; converged is False only for "max_iter"."""


def lbfgs(f, x0, history=10, max_iter=1000, gtol=1e-4):
    """Two-loop L-BFGS over a closure f(x) -> (value, gradient) on flat fp64 vectors.  The first step is 1 / max(1, |g|);
    later steps start at 1 on the direction scaled by s^T y / y^T y.  Armijo backtracking (c1 = 1e-4, halving); a curvature
    pair is kept only when s^T y > 0.  Stops at max |g| <= gtol, at max_iter, or when the line search cannot find a decrease:
    at the precision of f nothing further can be gained, so that is a form of convergence and not an error."""
    c1, max_halvings = 1e-4, 60
    x = np.array(x0, dtype=np.float64).reshape(-1)
    fx, g = f(x)
    fx, g = float(fx), np.asarray(g, dtype=np.float64).reshape(-1)
    n_evals, n_iter, status = 1, 0, "max_iter"
    S, Y, rho = [], [], []
    while True:
        if not np.isfinite(fx) or np.max(np.abs(g)) <= gtol:
            status = "gtol" if np.isfinite(fx) else "precision"
            break
        if n_iter >= max_iter:
            break
        if S:
            q = g.copy()
            a = [0.0] * len(S)
            for i in range(len(S) - 1, -1, -1):
                a[i] = rho[i] * (S[i] @ q)
                q -= a[i] * Y[i]
            q *= (S[-1] @ Y[-1]) / (Y[-1] @ Y[-1])
            for i in range(len(S)):
                q += (a[i] - rho[i] * (Y[i] @ q)) * S[i]
            d = -q
        else:
            d = -g / max(1.0, float(np.linalg.norm(g)))
        gd = float(g @ d)
        if not gd < 0:                                   # not a descent direction (cannot happen with s^T y > 0 in exact arithmetic)
            S, Y, rho = [], [], []
            d = -g / max(1.0, float(np.linalg.norm(g)))
            gd = float(g @ d)
        step, found = 1.0, False
        for _ in range(max_halvings):
            x_new = x + step * d
            f_new, g_new = f(x_new)
            n_evals += 1
            if np.isfinite(f_new) and f_new <= fx + c1 * step * gd and f_new < fx:     # (a step that rounds to no decrease is none)
                found = True
                break
            step *= 0.5
        if not found:
            status = "precision"
            break
        g_new = np.asarray(g_new, dtype=np.float64).reshape(-1)
        s, yv = x_new - x, g_new - g
        sy = float(s @ yv)
        if sy > 0:
            S.append(s)
            Y.append(yv)
            rho.append(1.0 / sy)
            if len(S) > history:
                S.pop(0), Y.pop(0), rho.pop(0)
        x, fx, g = x_new, float(f_new), g_new
        n_iter += 1
    return LbfgsResult(x, fx, g, n_iter, n_evals, status != "max_iter", status)


def logistic_objective(X, y, W, C=1.0, class_weight=None, fit_intercept=True):
    """numpy fp64 restatement of what LogisticRegressionProbe minimises (scikit-learn's objective): X (N, D), y (N,) ints,
    W (n_classes, D + 1) with the intercept in the last column -> (value, gradient (n_classes, D + 1)).
    sum_r w[y_r] (lse(z_r) - z_r[y_r]) + |W[:, :D]|^2 / (2 C); rows with a target outside [0, n_classes) take no part."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y).astype(np.int64)
    W = np.asarray(W, dtype=np.float64)
    nc = W.shape[0]
    ok = (y >= 0) & (y < nc)
    yc = np.where(ok, y, 0)
    w = np.where(ok, 1.0 if class_weight is None else np.asarray(class_weight, dtype=np.float64)[yc], 0.0)
    Z = X @ W[:, :-1].T + W[:, -1]
    m = Z.max(axis=1, keepdims=True)
    E = np.exp(Z - m)
    ssum = E.sum(axis=1, keepdims=True)
    rows = np.arange(len(y))
    loss = float(np.sum(w * (np.log(ssum[:, 0]) + (m[:, 0] - Z[rows, yc]))))
    R = E / ssum
    R[rows, yc] -= 1.0
    R *= w[:, None]
    grad = np.concatenate([R.T @ X, R.sum(axis=0)[:, None]], axis=1)
    loss += float(np.sum(W[:, :-1] ** 2)) / (2.0 * C)
    grad[:, :-1] += W[:, :-1] / C
    if not fit_intercept:
        grad[:, -1] = 0.0
    return loss, grad


# ----------------------------------------------------------------------------------------------------- device halves
def _f32_on(a, device):
    """A host fp64 array as a fresh fp32 device tensor with canonical strides (a (1, D) numpy array may carry any row stride)."""
    t = torch.empty(a.shape, dtype=torch.float32, device=device)
    t.copy_(torch.from_numpy(np.asarray(a, dtype=np.float64)))
    return t


def probe_gram(X, Y=None, out=None, accumulate=False):
    """G = Z^T Z (fp64, (D + 1 + K)^2) for Z = [X | 1 | Y] in one call of msn_probe_gram; with `out` and accumulate=True the
    product is added to what `out` holds.  Enqueue only: no allocation beyond the scratch, no synchronisation."""
    X = rows_on_gpu(X, "probe_gram", "embeddings")
    N, D = X.shape
    K = 0
    if Y is not None:
        if Y.device != X.device:
            raise _lib.MsnHipError("probe_gram: targets must live on the GPU next to the embeddings; there is no CPU path")
        Y = Y.detach()
        Y = Y.reshape(N, 1) if Y.dim() == 1 else Y
        if Y.dim() != 2 or Y.shape[0] != N or Y.dtype != torch.float32:
            raise ValueError(f"probe_gram: targets must be float32 ({N},) or ({N}, K) (got {Y.dtype} {tuple(Y.shape)})")
        K = Y.shape[1]
        if (Y.stride(1) != 1 and K > 1) or Y.stride(0) < K:
            Y = Y.contiguous()
    M = D + 1 + K
    if out is None:
        if accumulate:
            raise ValueError("probe_gram: accumulate needs the matrix to add to")
        out = torch.empty((M, M), dtype=torch.float64, device=X.device)
    elif out.shape != (M, M) or out.dtype != torch.float64 or out.device != X.device or not out.is_contiguous():
        raise ValueError(f"probe_gram: out must be a contiguous float64 ({M}, {M}) matrix on {X.device}")
    L = lib()
    nb = L.msn_probe_gram_workspace_bytes(N, D, K)
    ws = workspace(nb, X.device)
    check(L.msn_probe_gram(ptr(X), ld(X), ptr(Y if K else None), ld(Y) if K else 0, N, D, K, ptr(out), 1 if accumulate else 0,
                           ptr(ws), ws.numel(), stream_ptr()), "msn_probe_gram")
    return out


def logreg_loss_grad(X, y, W, class_weight=None, out=None):
    """out (1 + C (D + 1) doubles on the device) = {loss, gradient} of the unregularised multinomial logistic objective at
    W (C, D + 1) fp64 (msn_logreg_loss_grad).  Enqueue only."""
    X = rows_on_gpu(X, "logreg_loss_grad", "embeddings")
    N, D = X.shape
    if W.dim() != 2 or W.shape[1] != D + 1 or W.dtype != torch.float64 or W.device != X.device or not W.is_contiguous():
        raise ValueError(f"logreg_loss_grad: W must be a contiguous float64 (C, {D + 1}) matrix on {X.device}")
    C = W.shape[0]
    if y.shape != (N,) or y.dtype != torch.int64 or y.device != X.device:
        raise ValueError(f"logreg_loss_grad: targets must be int64 of shape ({N},) on {X.device}")
    y = y.contiguous()
    if class_weight is not None and (class_weight.shape != (C,) or class_weight.dtype != torch.float64
                                     or class_weight.device != X.device or not class_weight.is_contiguous()):
        raise ValueError(f"logreg_loss_grad: class_weight must be float64 of shape ({C},) on {X.device}")
    if out is None:
        out = torch.empty(1 + C * (D + 1), dtype=torch.float64, device=X.device)
    L = lib()
    nb = L.msn_logreg_workspace_bytes(N, D, C)
    ws = workspace(nb, X.device)
    check(L.msn_logreg_loss_grad(ptr(X), ld(X), ptr(y), ptr(class_weight), N, D, C, ptr(W), ptr(out), ptr(ws), ws.numel(),
                                 stream_ptr()), "msn_logreg_loss_grad")
    return out


class LinearRegressionProbe:
    """LinearRegression (alpha = 0) / Ridge (alpha > 0) on embeddings, fitted from sums over rows: partial_fit(X, Y) per
    validation batch is one Gram call on the device, solve() copies the (D + 1 + K)^2 matrix once and solves on the host."""

    def __init__(self, alpha=0.0, fit_intercept=True):
        if alpha < 0:
            raise ValueError("LinearRegressionProbe: alpha must not be negative")
        self.alpha, self.fit_intercept = float(alpha), bool(fit_intercept)
        self.reset()

    def reset(self):
        self.gram = None                     # (D + 1 + K)^2 fp64 on the device; several ranks all-reduce it before solve()
        self.coef_ = self.intercept_ = None
        self._shape = self._w = self._b = None

    def partial_fit(self, X, Y):
        X = rows_on_gpu(X, "LinearRegressionProbe.partial_fit", "embeddings")
        if not isinstance(Y, torch.Tensor) or Y.device != X.device:
            raise _lib.MsnHipError("LinearRegressionProbe.partial_fit: targets must live on the GPU next to the embeddings; "
                                   "there is no CPU path")
        flat = Y.dim() == 1
        Y2 = Y.detach().to(torch.float32)
        Y2 = Y2.reshape(-1, 1) if flat else Y2
        shape = (X.shape[1], Y2.shape[1], flat)
        if self._shape is not None and shape != self._shape:
            raise ValueError(f"LinearRegressionProbe.partial_fit: (D, K) changed from {self._shape[:2]} to {shape[:2]}")
        if not 1 <= shape[1] <= MAX_K:
            raise ValueError(f"LinearRegressionProbe: 1 to {MAX_K} target columns (got {shape[1]})")
        self.gram = probe_gram(X, Y2, out=self.gram, accumulate=self.gram is not None)
        self._shape = shape
        self.coef_ = self.intercept_ = self._w = self._b = None
        return self

    def fit(self, X, Y):
        self.reset()
        return self.partial_fit(X, Y).solve()

    def solve(self):
        if self.gram is None:
            raise ValueError("LinearRegressionProbe.solve: nothing fitted yet")
        D, K, flat = self._shape
        coef, intercept = solve_normal_equations(self.gram.cpu().numpy(), D, K, self.alpha, self.fit_intercept)
        self._w, self._b = _f32_on(coef, self.gram.device), _f32_on(intercept, self.gram.device)
        self.coef_, self.intercept_ = (coef[0], float(intercept[0])) if flat else (coef, intercept)
        return self

    def predict(self, X):
        if self._w is None:
            self.solve()
        from .functional import linear
        X = rows_on_gpu(X, "LinearRegressionProbe.predict", "embeddings")
        with torch.no_grad():
            out = linear(X.contiguous(), self._w, self._b)
        return out[:, 0] if self._shape[2] else out


class LogisticRegressionProbe:
    """LogisticRegression (multinomial, L2, lbfgs) on embeddings: fit(X, y) minimises scikit-learn's objective
    sum_r w[y_r] l_r + |W|^2 / (2 C) with the intercept unpenalised, from zero.  W and the gradient are fp64 on both sides; an
    evaluation uploads W in one copy, makes the kernel's two launches and downloads 1 + C (D + 1) doubles in one copy."""

    def __init__(self, C=1.0, n_classes=None, class_weight=None, max_iter=1000, tol=1e-4, fit_intercept=True):
        if C <= 0:
            raise ValueError("LogisticRegressionProbe: C must be positive")
        self.C, self.n_classes, self.class_weight = float(C), n_classes, class_weight
        self.max_iter, self.tol, self.fit_intercept = int(max_iter), float(tol), bool(fit_intercept)
        self.coef_ = self.intercept_ = self.n_iter_ = self.n_evals_ = self.converged_ = None
        self._w = self._b = None

    def fit(self, X, y):
        X = rows_on_gpu(X, "LogisticRegressionProbe.fit", "embeddings")
        if not isinstance(y, torch.Tensor) or y.device != X.device:
            raise _lib.MsnHipError("LogisticRegressionProbe.fit: targets must live on the GPU next to the embeddings; "
                                   "there is no CPU path")
        y = y.detach().to(torch.int64).contiguous()
        N, D = X.shape
        nc = int(self.n_classes) if self.n_classes is not None else int(y.max().item()) + 1
        if nc < 2 or D > MAX_D or nc * (D + 1) > MAX_W:
            raise _lib.MsnHipError(f"LogisticRegressionProbe: needs n_classes >= 2, D <= {MAX_D} and n_classes (D + 1) <= {MAX_W} "
                                   f"(got n_classes = {nc}, D = {D})")
        cw = None
        if self.class_weight is not None:
            cw = torch.as_tensor(np.asarray(self.class_weight.detach().cpu() if isinstance(self.class_weight, torch.Tensor)
                                            else self.class_weight, dtype=np.float64)).to(X.device)
            if cw.shape != (nc,):
                raise ValueError(f"LogisticRegressionProbe: class_weight must have shape ({nc},)")
        W_dev = torch.empty((nc, D + 1), dtype=torch.float64, device=X.device)
        out_dev = torch.empty(1 + nc * (D + 1), dtype=torch.float64, device=X.device)
        reg = 1.0 / self.C

        def f(w):
            Wh = w.reshape(nc, D + 1)
            W_dev.copy_(torch.from_numpy(Wh))                              # one copy up
            logreg_loss_grad(X, y, W_dev, cw, out=out_dev)
            o = out_dev.cpu().numpy()                                      # one copy down (the synchronisation)
            grad = o[1:].reshape(nc, D + 1).copy()
            grad[:, :D] += reg * Wh[:, :D]
            if not self.fit_intercept:
                grad[:, D] = 0.0
            return float(o[0]) + 0.5 * reg * float(np.sum(Wh[:, :D] ** 2)), grad.reshape(-1)

        res = lbfgs(f, np.zeros(nc * (D + 1)), max_iter=self.max_iter, gtol=self.tol)
        Wh = res.x.reshape(nc, D + 1)
        self.coef_, self.intercept_ = Wh[:, :D].copy(), Wh[:, D].copy()
        self.n_iter_, self.n_evals_, self.converged_ = res.n_iter, res.n_evals, res.converged
        self.objective_ = res.fun
        self._w, self._b = _f32_on(self.coef_, X.device), _f32_on(self.intercept_, X.device)
        return self

    def decision_function(self, X):
        if self._w is None:
            raise ValueError("LogisticRegressionProbe: not fitted")
        from .functional import linear
        X = rows_on_gpu(X, "LogisticRegressionProbe.decision_function", "embeddings")
        with torch.no_grad():
            return linear(X.contiguous(), self._w, self._b)

    def predict(self, X):
        """Class per row, int32 (first maximal index, as torch.argmax)."""
        from .models_finetune import argmax_rows
        return argmax_rows(self.decision_function(X))


# ------------------------------------------------------------------------------------------------ host: kNN restated
def _weights_code(weights, who):
    if weights not in ("uniform", "distance"):
        raise ValueError(f"{who}: weights must be 'uniform' or 'distance' (got {weights!r})")
    return 1 if weights == "distance" else 0


def knn_reference(Q, X, k, self_offset=-1):
    """numpy fp64 restatement of msn_knn_search: (idx int32 (Nq, k), dist2 fp64 (Nq, k)).  Distances in the direct form
    sum_c (q_c - x_c)^2; order by np.argsort(kind="stable"), so the lower index comes first among equal distances; with
    self_offset >= 0 the row i + self_offset is no candidate of query i."""
    Q = np.asarray(Q, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    k, self_offset = int(k), int(self_offset)
    if Q.ndim != 2 or X.ndim != 2 or Q.shape[1] != X.shape[1]:
        raise ValueError(f"knn_reference: Q (Nq, D) and X (Nx, D) needed (got {Q.shape} and {X.shape})")
    if not 1 <= k <= len(X) - (1 if self_offset >= 0 else 0):
        raise ValueError(f"knn_reference: k = {k} outside 1..{len(X) - (1 if self_offset >= 0 else 0)}")
    idx = np.empty((len(Q), k), dtype=np.int32)
    dist2 = np.empty((len(Q), k), dtype=np.float64)
    for i, q in enumerate(Q):
        d = ((X - q) ** 2).sum(axis=1)
        order = np.argsort(d, kind="stable")
        if self_offset >= 0:
            order = order[order != i + self_offset]
        idx[i] = order[:k]
        dist2[i] = d[order[:k]]
    return idx, dist2


def knn_predict_reference(idx, dist2, targets, weights="uniform", task="regression", n_classes=None):
    """numpy fp64 restatement of the kNN prediction kernels over a search's (idx, dist2).  Weights: 1 (uniform) or
    1 / sqrt(dist2) (distance); a query with a zero distance among its k gives its zero-distance neighbours weight 1 and the
    others 0 (scikit-learn's rule).  Sums run in neighbour order.
    task="regression": targets (Nx,) or (Nx, K) -> fp64 predictions (Nq,) or (Nq, K), sum w y / sum w.
    task="classification": targets (Nx,) ints -> (classes int32 (Nq,), votes fp64 (Nq, n_classes)); the lowest class wins
    equal votes; a label outside [0, n_classes) counts for no class."""
    code = _weights_code(weights, "knn_predict_reference")
    idx = np.asarray(idx).astype(np.int64)
    dist2 = np.asarray(dist2, dtype=np.float64)
    nq, k = idx.shape
    if code:
        zero = dist2 == 0.0
        with np.errstate(divide="ignore"):
            w = np.where(zero.any(axis=1, keepdims=True), zero.astype(np.float64), 1.0 / np.sqrt(dist2))
    else:
        w = np.ones((nq, k))
    if task == "regression":
        Y = np.asarray(targets, dtype=np.float64)
        flat = Y.ndim == 1
        Y = Y.reshape(len(Y), -1)
        num = np.zeros((nq, Y.shape[1]))
        den = np.zeros(nq)
        for t in range(k):
            num += w[:, t, None] * Y[idx[:, t]]
            den += w[:, t]
        out = num / den[:, None]
        return out[:, 0] if flat else out
    if task != "classification":
        raise ValueError(f"knn_predict_reference: task must be 'regression' or 'classification' (got {task!r})")
    y = np.asarray(targets).astype(np.int64)
    C = int(n_classes) if n_classes is not None else int(y.max()) + 1
    votes = np.zeros((nq, C))
    rows = np.arange(nq)
    for t in range(k):
        lab = y[idx[:, t]]
        ok = (lab >= 0) & (lab < C)
        votes[rows[ok], lab[ok]] += w[ok, t]
    return votes.argmax(axis=1).astype(np.int32), votes


# ----------------------------------------------------------------------------------------------------- device: kNN
KNN_MAX_K = 64
KNN_MAX_CLASSES = 1024


def _knn_metric(metric, who):
    if metric not in ("euclidean", "cosine"):
        raise ValueError(f"{who}: metric must be 'euclidean' or 'cosine' (got {metric!r})")
    return metric


def _unit_rows(X):
    from . import ops
    return ops.l2norm_fwd(X.contiguous())[0]


def _knn_search_sq(Q, X, k, self_offset):
    """(idx int32 (Nq, k), dist2 fp64 (Nq, k)) of msn_knn_search over checked device tensors.  Enqueue only."""
    if Q.device != X.device:
        raise _lib.MsnHipError("knn_search: queries and training set must live on the same GPU")
    if Q.shape[1] != X.shape[1]:
        raise ValueError(f"knn_search: queries have {Q.shape[1]} columns, the training set {X.shape[1]}")
    (Nq, D), Nx = Q.shape, X.shape[0]
    idx = torch.empty((Nq, k), dtype=torch.int32, device=Q.device)
    dist2 = torch.empty((Nq, k), dtype=torch.float64, device=Q.device)
    L = lib()
    ws = workspace(L.msn_knn_workspace_bytes(Nq, Nx, D, k), Q.device)
    check(L.msn_knn_search(ptr(Q), ld(Q), Nq, ptr(X), ld(X), Nx, D, k, self_offset, ptr(idx), ptr(dist2), ptr(ws),
                           ws.numel(), stream_ptr()), "msn_knn_search")
    return idx, dist2


def _self_offset(exclude_self):
    if exclude_self is False or exclude_self is None:
        return -1
    if exclude_self is True:
        return 0
    if int(exclude_self) < 0:
        raise ValueError(f"knn_search: exclude_self must be False or the row offset of the queries (got {exclude_self!r})")
    return int(exclude_self)


def knn_search(Q, X, k, metric="euclidean", exclude_self=False, return_squared=False):
    """The k nearest rows of X (Nx, D) for every row of Q (Nq, D), exactly: (idx int32 (Nq, k), dist fp64 (Nq, k)), ascending,
    ties by the lower index (msn_knn_search).  metric="euclidean" returns sqrt(d^2) as scikit-learn does; "cosine"
    L2-normalises both sides first (ops.l2norm_fwd, which takes D a multiple of 4) and returns 1 - cos = d^2 / 2.  return_squared=True returns the kernel's
    d^2 untouched (of the normalised rows for "cosine").  exclude_self: False, or the offset o of the queries in the training
    set (True = 0): query i never finds row i + o -- leave-one-out for Q = X[o : o + n].  Enqueue only."""
    _knn_metric(metric, "knn_search")
    same = Q is X
    Q = rows_on_gpu(Q, "knn_search", "embeddings")
    X = Q if same else rows_on_gpu(X, "knn_search", "embeddings")
    if metric == "cosine":
        Q = _unit_rows(Q)
        X = Q if same else _unit_rows(X)
    idx, d2 = _knn_search_sq(Q, X, int(k), _self_offset(exclude_self))
    if return_squared:
        return idx, d2
    return idx, (d2 * 0.5 if metric == "cosine" else d2.sqrt())


class _KNeighborsProbe:
    """What the two kNN probes share: the training set kept on the device (unit rows for metric="cosine") and the search."""

    def __init__(self, n_neighbors=5, weights="uniform", metric="euclidean"):
        who = type(self).__name__
        if not 1 <= int(n_neighbors) <= KNN_MAX_K:
            raise ValueError(f"{who}: n_neighbors must be in 1..{KNN_MAX_K} (got {n_neighbors})")
        self.n_neighbors, self.weights, self.metric = int(n_neighbors), weights, _knn_metric(metric, who)
        self._wcode = _weights_code(weights, who)
        self._X = self._t = None

    def _fit_x(self, X):
        X = rows_on_gpu(X, f"{type(self).__name__}.fit", "embeddings")        # a reference: contiguous input is not copied
        if X.shape[1] > MAX_D:
            raise _lib.MsnHipError(f"{type(self).__name__}: D <= {MAX_D} (got {X.shape[1]})")
        self._X = _unit_rows(X) if self.metric == "cosine" else X
        return X

    def _targets_on(self, X, Y):
        if not isinstance(Y, torch.Tensor) or Y.device != X.device:
            raise _lib.MsnHipError(f"{type(self).__name__}.fit: targets must live on the GPU next to the embeddings; "
                                   "there is no CPU path")
        if Y.shape[0] != X.shape[0]:
            raise ValueError(f"{type(self).__name__}.fit: {X.shape[0]} rows of embeddings, {Y.shape[0]} targets")
        return Y.detach()

    def _search(self, X, k):
        """(idx, d^2) for the rows of X, or leave-one-out over the training set for X = None."""
        if self._X is None:
            raise ValueError(f"{type(self).__name__}: not fitted")
        if X is None:
            return _knn_search_sq(self._X, self._X, k, 0)
        Q = rows_on_gpu(X, f"{type(self).__name__}", "embeddings")
        return _knn_search_sq(_unit_rows(Q) if self.metric == "cosine" else Q, self._X, k, -1)

    def kneighbors(self, X=None, n_neighbors=None, return_distance=True):
        """scikit-learn's call: (distances fp64 (Nq, k), indices int32 (Nq, k)), or the indices alone with
        return_distance=False.  X = None searches the training set itself, every row without itself."""
        idx, d2 = self._search(X, self.n_neighbors if n_neighbors is None else int(n_neighbors))
        if not return_distance:
            return idx
        return (d2 * 0.5 if self.metric == "cosine" else d2.sqrt()), idx

    def _neighbours(self, X):
        """(idx, the squared distance the prediction kernels weigh by) at n_neighbors."""
        idx, d2 = self._search(X, self.n_neighbors)
        if self.metric == "cosine" and self._wcode:
            d2 = (d2 * 0.5).square()                         # the kernels weigh by 1 / sqrt: the distance here is 1 - cos
        return idx, d2


class KNeighborsRegressorProbe(_KNeighborsProbe):
    """KNeighborsRegressor on embeddings: exact search (msn_knn_search), then the weighted mean of the neighbours' targets in
    fp64, rounded once to fp32 (msn_knn_predict_regression).  predict() / kneighbors() without X are leave-one-out over the
    training set.  Approximate search, other metrics, k > 64, radius_neighbors and sample weights are not built."""

    def fit(self, X, Y):
        X = self._fit_x(X)
        Y = self._targets_on(X, Y)
        self._flat = Y.dim() == 1
        Y2 = Y.to(torch.float32)
        Y2 = Y2.reshape(-1, 1) if self._flat else Y2
        if Y2.dim() != 2 or not 1 <= Y2.shape[1] <= MAX_K:
            raise ValueError(f"KNeighborsRegressorProbe: 1 to {MAX_K} target columns (got {tuple(Y.shape)})")
        if (Y2.stride(1) != 1 and Y2.shape[1] > 1) or Y2.stride(0) < Y2.shape[1]:
            Y2 = Y2.contiguous()
        self._t = Y2
        return self

    def predict(self, X=None):
        idx, d2 = self._neighbours(X)
        Nq, k = idx.shape
        K = self._t.shape[1]
        out = torch.empty((Nq, K), dtype=torch.float32, device=idx.device)
        check(lib().msn_knn_predict_regression(ptr(idx), ptr(d2), Nq, k, ptr(self._t), ld(self._t), K, self._wcode, ptr(out), K,
                                               stream_ptr()), "msn_knn_predict_regression")
        return out[:, 0] if self._flat else out


class KNeighborsClassifierProbe(_KNeighborsProbe):
    """KNeighborsClassifier on embeddings: exact search, then the weighted vote in fp64 (msn_knn_predict_classes); the lowest
    class wins equal votes, as scikit-learn's mode does.  predict returns int32 classes, like LogisticRegressionProbe."""

    def __init__(self, n_neighbors=5, weights="uniform", metric="euclidean", n_classes=None):
        super().__init__(n_neighbors, weights, metric)
        self.n_classes = n_classes

    def fit(self, X, y):
        X = self._fit_x(X)
        y = self._targets_on(X, y)
        if y.dim() != 1:
            raise ValueError(f"KNeighborsClassifierProbe.fit: labels must have shape ({X.shape[0]},) (got {tuple(y.shape)})")
        y = y.to(torch.int64).contiguous()
        lo, hi = int(y.min().item()), int(y.max().item())
        nc = int(self.n_classes) if self.n_classes is not None else hi + 1
        if lo < 0 or hi >= nc or not 1 <= nc <= KNN_MAX_CLASSES:
            raise _lib.MsnHipError(f"KNeighborsClassifierProbe: labels must lie in [0, n_classes) with n_classes <= "
                                   f"{KNN_MAX_CLASSES} (got labels {lo}..{hi}, n_classes = {nc})")
        self._t, self._nc = y, nc
        return self

    def _vote(self, X, want_proba):
        idx, d2 = self._neighbours(X)
        Nq, k = idx.shape
        classes = torch.empty(Nq, dtype=torch.int32, device=idx.device)
        proba = torch.empty((Nq, self._nc), dtype=torch.float32, device=idx.device) if want_proba else None
        check(lib().msn_knn_predict_classes(ptr(idx), ptr(d2), Nq, k, ptr(self._t), self._nc, self._wcode, ptr(classes),
                                            ptr(proba), stream_ptr()), "msn_knn_predict_classes")
        return classes, proba

    def predict(self, X=None):
        return self._vote(X, False)[0]

    def predict_proba(self, X=None):
        """(Nq, n_classes) fp32: each class's share of the votes."""
        return self._vote(X, True)[1]
