"""Float64 numpy restatement of Optimizer::OptimizeSim3 (reference src/Optimizer.cc:4195-4494): what the tests
of orb_optimize_sim3 compare against.  Written from the reference's sources:

  lm_optimize     SparseOptimizer::optimize(n) with OptimizationAlgorithmLevenberg::solve
                  (core/optimization_algorithm_levenberg.cpp:61-194) and LinearSolverDense: ONE function over an
                  edge model (errors / build / oplus / state).  PoseModel (the mono only-pose edge with
                  PoseOptimization's four rounds) pins it to oracle.pose_optimization; Sim3Model is the model
                  under test.
  Sim3            g2o::Sim3 (types/sim3.h:70-142, 144, 233, 266): exp with its four eps branches, map, inverse, *.
  Sim3Model       VertexSim3Expmap::oplusImpl (_fix_scale zeroes update[6]), EdgeSim3ProjectXYZ and
                  EdgeInverseSim3ProjectXYZ, g2o's central differences (base_binary_edge.hpp:131-205, delta 1e-9),
                  constructQuadraticForm with RobustKernelHuber (float dsqr).
  optimize_sim3   the schedule: optimize(5), the first cull on the stored errors, the < 10 exit, optimize(10 | 5)
                  without kernels, the second cull; with each cull's decisive pairs.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
DBL_MAX = np.finfo(np.float64).max
DELTA = 1e-9
DECISIVE_STEP = 1e-6     # the project's pose bar


# ---- the controller ------------------------------------------------------------------------------------------
def ldlt_solve(S, b):
    """Dense LDL^T without pivoting (Eigen::LDLT up to rounding).  Returns (isPositive, x); x = 0 on failure."""
    n = len(b)
    L = np.zeros((n, n))
    d = np.zeros(n)
    ok = True
    with np.errstate(all="ignore"):
        for j in range(n):
            dj = S[j, j] - np.sum(L[j, :j] * L[j, :j] * d[:j])
            ok = ok and dj > 0
            d[j] = dj
            for i in range(j + 1, n):
                L[i, j] = (S[j, i] - np.sum(L[i, :j] * L[j, :j] * d[:j])) / dj
        x = np.array(b, np.float64)
        for i in range(n):
            x[i] -= np.sum(L[i, :i] * x[:i])
        x /= d
        for i in range(n - 1, -1, -1):
            x[i] -= np.sum(L[i + 1:, i] * x[i + 1:])
    if not ok:
        x = np.zeros(n)
    return ok, x


def lm_optimize(model, iterations):
    """optimize(iterations).  model: any_active(), errors() (computeActiveErrors; returns activeRobustChi2 and
    keeps every active edge's error), build() -> (H, b) on the kept errors, state() / set_state(), oplus(x).
    Returns the number of trials (for the tests)."""
    if not model.any_active():
        return 0
    lam, ni, nbad, trials = 0.0, 2.0, 0, 0
    for it in range(iterations):
        current = model.errors()
        ini = current
        H, b = model.build()
        if it == 0:                                  # computeLambdaInit: tau * max |diag H|
            lam, ni, nbad = 1e-5 * float(np.max(np.abs(np.diag(H)))), 2.0, 0
        qmax = 0
        while True:
            backup = model.state()
            ok, x = ldlt_solve(H + lam * np.eye(len(b)), b)
            model.oplus(x)                           # (may zero entries of x in place, as oplusImpl does)
            temp = model.errors()
            trials += 1
            if not ok:
                temp = DBL_MAX
            with np.errstate(all="ignore"):
                rho = (current - temp) / (float(np.sum(x * (lam * x + b))) + 1e-3)
            if rho > 0 and np.isfinite(temp):
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                current = temp
            else:
                lam *= ni
                ni *= 2
                model.set_state(backup)
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        if qmax == 10 or rho == 0:
            return trials
        nbad = nbad + 1 if (ini - current) * 1e3 < ini else 0
        if nbad >= 3:
            return trials
    return trials


class Huber:
    """RobustKernelHuber: double delta, float dsqr (robust_kernel_impl.cpp:78-91)."""

    def __init__(self, delta_f32):
        self.delta = float(f32(delta_f32))
        self.dsqr = float(f32(self.delta * self.delta))

    def rho(self, e):
        e = np.asarray(e, np.float64)
        small = e <= self.dsqr
        with np.errstate(all="ignore"):
            sq = np.sqrt(e)
            return np.where(small, e, 2 * sq * self.delta - self.dsqr), np.where(small, 1.0, self.delta / sq)


# ---- the controller's anchor: PoseOptimization's mono edge ----------------------------------------------------
def _skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def quat_to_rot(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rot_to_quat(m):
    """Eigen's Quaterniond(Matrix3d) (x y z w)."""
    q = np.zeros(4)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return q


def se3_exp(x):
    """SE3Quat::exp: (R, t) of (omega, upsilon)."""
    w, u = x[:3], x[3:]
    th = float(np.linalg.norm(w))
    O = _skew(w)
    O2 = O @ O
    if th < 0.00001:
        R = np.eye(3) + O + O2
        V = R
    else:
        R = np.eye(3) + np.sin(th) / th * O + (1 - np.cos(th)) / (th * th) * O2
        V = np.eye(3) + (1 - np.cos(th)) / (th * th) * O + (th - np.sin(th)) / (th ** 3) * O2
    return R, V @ u


class PoseModel:
    """EdgeSE3ProjectXYZOnlyPose on one VertexSE3Expmap (mono edges only)."""

    def __init__(self, frame, edges):
        self.E = edges
        self.cam = [float(frame["cam"][k]) for k in ("fx", "fy", "cx", "cy")]
        self.level = np.zeros(len(edges), bool)
        self.err = np.zeros((len(edges), 2))
        self.robust = True
        self.huber = Huber(np.sqrt(5.991))
        self.info = edges["inv_sigma2"].astype(np.float64)
        self.set_pose(frame["pose"])

    def set_pose(self, p):
        self.R, self.t = quat_to_rot(np.asarray(p[3:], np.float64)), np.array(p[:3], np.float64)

    def pose(self):
        return np.concatenate([self.t, rot_to_quat(self.R)])

    def state(self):
        return self.R.copy(), self.t.copy()

    def set_state(self, s):
        self.R, self.t = s[0].copy(), s[1].copy()

    def oplus(self, x):
        R, t = se3_exp(x)
        self.R, self.t = R @ self.R, R @ self.t + t

    def any_active(self):
        return bool((~self.level).any())

    def edge_errors(self):
        fx, fy, cx, cy = self.cam
        Xc = self.E["xw"] @ self.R.T + self.t
        e = np.stack([self.E["obs"][:, 0] - (fx * Xc[:, 0] / Xc[:, 2] + cx),
                      self.E["obs"][:, 1] - (fy * Xc[:, 1] / Xc[:, 2] + cy)], 1)
        return e, Xc

    def chi2(self):
        return self.info * (self.err ** 2).sum(1)

    def errors(self):
        e, _ = self.edge_errors()
        a = ~self.level
        self.err[a] = e[a]
        c = self.chi2()[a]
        return float(np.sum(self.huber.rho(c)[0] if self.robust else c))

    def build(self):
        fx, fy = self.cam[:2]
        a = ~self.level
        _, Xc = self.edge_errors()
        x, y, z = Xc[a, 0], Xc[a, 1], Xc[a, 2]
        zero = np.zeros_like(x)
        # -projectJac * [-[Xc]x | I] (src/OptimizableTypes.cpp:58-73)
        j00, j02, j11, j12 = -fx / z, fx * x / (z * z), -fy / z, fy * y / (z * z)
        D = np.zeros((len(x), 3, 6))
        D[:, 0, 1], D[:, 0, 2], D[:, 1, 0], D[:, 1, 2], D[:, 2, 0], D[:, 2, 1] = z, -y, -z, x, y, -x
        D[:, 0, 3] = D[:, 1, 4] = D[:, 2, 5] = 1
        P = np.stack([np.stack([j00, zero, j02], 1), np.stack([zero, j11, j12], 1)], 1)
        J = P @ D
        rho1 = self.huber.rho(self.chi2()[a])[1] if self.robust else np.ones(len(x))
        w = rho1 * self.info[a]
        H = np.einsum("nri,n,nrj->ij", J, w, J)
        b = -np.einsum("nri,n,nr->i", J, w, self.err[a])
        return H, b


def pose_optimization(frames, edges):
    """PoseOptimization's schedule (src/Optimizer.cc:278-386) over lm_optimize, mono edges only.
    Returns (poses [n, 7], outlier flags per edge, inliers per frame) like oracle.pose_optimization."""
    poses = np.zeros((len(frames), 7))
    outl = np.zeros(len(edges), bool)
    inl = np.zeros(len(frames), np.int32)
    for fi, F in enumerate(frames):
        E = edges[F["edge_begin"]:F["edge_begin"] + F["n_edges"]]
        assert not E["stereo"].any()
        poses[fi] = F["pose"]
        n = len(E)
        if n < 3:
            continue
        M = PoseModel(F, E)
        nbad = 0
        for it in range(4):
            M.set_pose(F["pose"])
            lm_optimize(M, 10)
            e, _ = M.edge_errors()
            M.err[M.level] = e[M.level]              # an outlier's computeError() at the round's final pose
            M.level = M.chi2().astype(f32) > f32(5.991)
            nbad = int(M.level.sum())
            if it == 2:
                M.robust = False
            if n < 10:
                break
        poses[fi], outl[F["edge_begin"]:F["edge_begin"] + n], inl[fi] = M.pose(), M.level, n - nbad
    return poses, outl, inl


# ---- g2o::Sim3 -----------------------------------------------------------------------------------------------
def qrotate(q, v):
    """Eigen's Quaternion * Vector3 (q: x y z w, not assumed unit); v [..., 3]."""
    qv = q[:3]
    uv = 2 * np.cross(qv, v)
    return v + q[3] * uv + np.cross(qv, uv)


def qmul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


class Sim3:
    def __init__(self, q, t, s):
        self.q, self.t, self.s = np.array(q, np.float64), np.array(t, np.float64), float(s)

    @staticmethod
    def from_vector(v):
        """operator[] order: qx qy qz qw tx ty tz s."""
        return Sim3(v[:4], v[4:7], v[7])

    def vector(self):
        return np.concatenate([self.q, self.t, [self.s]])

    @staticmethod
    def exp(update, return_branch=False):
        """Sim3(const Vector7d& update) (sim3.h:70-142)."""
        omega, upsilon, sigma = np.array(update[:3], np.float64), np.array(update[3:6], np.float64), float(update[6])
        theta = float(np.sqrt(np.sum(omega * omega)))
        O = _skew(omega)
        s = float(np.exp(sigma))
        O2 = O @ O
        I = np.eye(3)
        eps = 0.00001
        if abs(sigma) < eps:
            C = 1.0
            if theta < eps:
                A, B, branch = 1. / 2., 1. / 6., 0
                R = I + O + O @ O
            else:
                theta2 = theta * theta
                A = (1 - np.cos(theta)) / theta2
                B = (theta - np.sin(theta)) / (theta2 * theta)
                R = I + np.sin(theta) / theta * O + (1 - np.cos(theta)) / (theta * theta) * O2
                branch = 1
        else:
            C = (s - 1) / sigma
            if theta < eps:
                sigma2 = sigma * sigma
                A = ((sigma - 1) * s + 1) / sigma2
                B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
                R = I + O + O2
                branch = 2
            else:
                R = I + np.sin(theta) / theta * O + (1 - np.cos(theta)) / (theta * theta) * O2
                a, b = s * np.sin(theta), s * np.cos(theta)
                theta2, sigma2 = theta * theta, sigma * sigma
                c = theta2 + sigma2
                A = (a * sigma + (1 - b) * theta) / (theta * c)
                B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
                branch = 3
        W = A * O + B * O2 + C * I
        S = Sim3(rot_to_quat(R), W @ upsilon, s)
        return (S, branch) if return_branch else S

    def map(self, X):
        return self.s * qrotate(self.q, X) + self.t

    def inverse(self):
        qc = np.array([-self.q[0], -self.q[1], -self.q[2], self.q[3]])
        return Sim3(qc, qrotate(qc, (-1. / self.s) * self.t), 1. / self.s)

    def __mul__(self, o):
        return Sim3(qmul(self.q, o.q), self.s * qrotate(self.q, o.t) + self.t, self.s * o.s)


def project(cam, X):
    """Pinhole::project(Vector3d): the float parameters promoted."""
    fx, fy, cx, cy = (float(f32(c)) for c in cam)
    return np.stack([fx * X[..., 0] / X[..., 2] + cx, fy * X[..., 1] / X[..., 2] + cy], -1)


# ---- the model under test -------------------------------------------------------------------------------------
class Sim3Model:
    """prob: a dict with p1c, p2c [n, 3] float64, obs1, obs2 [n, 2] float64, inv_sigma2_1, inv_sigma2_2 [n]
    float32, cam1, cam2 (fx fy cx cy), s12 [8], th2, fix_scale."""

    def __init__(self, prob):
        g = lambda k, d: np.ascontiguousarray(prob[k], d)  # noqa: E731
        self.p1, self.p2, self.o1, self.o2 = (g(k, np.float64) for k in ("p1c", "p2c", "obs1", "obs2"))
        self.i1, self.i2 = g("inv_sigma2_1", f32).astype(np.float64), g("inv_sigma2_2", f32).astype(np.float64)
        self.n = len(self.p1)
        self.cam1, self.cam2 = prob["cam1"], prob["cam2"]
        self.fix = bool(prob["fix_scale"])
        self.th2 = float(f32(prob["th2"]))
        self.huber = Huber(np.sqrt(f32(prob["th2"])))   # const float deltaHuber = sqrt(th2)
        self.S = Sim3.from_vector(np.asarray(prob["s12"], np.float64))
        self.bad = np.zeros(self.n, bool)
        self.robust = True
        self.e12, self.e21 = np.zeros((self.n, 2)), np.zeros((self.n, 2))
        self.S_eval = self.S        # the last state errors() saw

    def state(self):
        return self.S

    def set_state(self, S):
        self.S = S

    def oplus_of(self, S, x):
        if self.fix:
            x[6] = 0
        return Sim3.exp(x) * S

    def oplus(self, x):
        self.S = self.oplus_of(self.S, x)

    def any_active(self):
        return bool((~self.bad).any())

    def edge_errors(self, S, idx=slice(None)):
        e12 = self.o1[idx] - project(self.cam1, S.map(self.p2[idx]))
        e21 = self.o2[idx] - project(self.cam2, S.inverse().map(self.p1[idx]))
        return e12, e21

    def chi2_at(self, S):
        e12, e21 = self.edge_errors(S)
        return self.i1 * (e12 ** 2).sum(1), self.i2 * (e21 ** 2).sum(1)

    def chi2(self):
        return self.i1 * (self.e12 ** 2).sum(1), self.i2 * (self.e21 ** 2).sum(1)

    def errors(self):
        a = ~self.bad
        e12, e21 = self.edge_errors(self.S)
        self.e12[a], self.e21[a] = e12[a], e21[a]
        self.S_eval = self.S
        c12, c21 = self.chi2()
        if self.robust:
            return float(np.sum(self.huber.rho(c12[a])[0]) + np.sum(self.huber.rho(c21[a])[0]))
        return float(np.sum(c12[a]) + np.sum(c21[a]))

    def jacobians(self, S, idx=slice(None)):
        """g2o's central differences: [n, 2, 7] for e12 and e21."""
        J12 = np.zeros((len(self.p1[idx]), 2, 7))
        J21 = np.zeros_like(J12)
        scalar = 1.0 / (2 * DELTA)
        for d in range(7):
            u = np.zeros(7)
            u[d] = DELTA
            ap, bp = self.edge_errors(self.oplus_of(S, u), idx)
            u = np.zeros(7)
            u[d] = -DELTA
            am, bm = self.edge_errors(self.oplus_of(S, u), idx)
            J12[:, :, d], J21[:, :, d] = scalar * (ap - am), scalar * (bp - bm)
        return J12, J21

    def build(self):
        a = ~self.bad
        J12, J21 = self.jacobians(self.S, a)
        c12, c21 = self.chi2()
        H, b = np.zeros((7, 7)), np.zeros(7)
        for J, e, c, info in ((J12, self.e12[a], c12[a], self.i1[a]), (J21, self.e21[a], c21[a], self.i2[a])):
            rho1 = self.huber.rho(c)[1] if self.robust else np.ones(len(c))
            w = rho1 * info
            H += np.einsum("nri,n,nrj->ij", J, w, J)
            b -= np.einsum("nri,n,nr->i", J, w, e)
        return H, b


def _classes_under_perturbation(M, S, th2):
    """bad-classification of every pair at S and at the 14 estimates exp(+-1e-6 e_d) * S."""
    out = []
    for k in range(-1, 14):
        u = np.zeros(7)
        if k >= 0:
            u[k >> 1] = -DECISIVE_STEP if k & 1 else DECISIVE_STEP
        c12, c21 = M.chi2_at(M.oplus_of(S, u))
        out.append((c12 > th2) | (c21 > th2))
    return np.array(out)


def optimize_sim3(prob):
    """Returns a dict: s12 [8], n_in, n_bad, inlier [n] bool, chi2_12, chi2_21 [n], and the decisiveness of
    each cull: decisive1 / decisive2 [n] bool (a pair's class is the same at the cull's estimate and under its 14
    perturbations by +-1e-6), decisive (the problem: every pair decisive at the first cull, so that nBad, nBad > 0
    and nCorrespondences - nBad < 10 are not in doubt), early (the < 10 exit)."""
    M = Sim3Model(prob)
    n, th2 = M.n, M.th2
    s_in = np.asarray(prob["s12"], np.float64).copy()
    res = {"s12": s_in, "n_in": 0, "n_bad": 0, "inlier": np.zeros(n, bool), "chi2_12": np.zeros(n),
           "chi2_21": np.zeros(n), "decisive1": np.ones(n, bool), "decisive2": np.ones(n, bool), "decisive": True,
           "early": True, "trials": [0, 0]}
    if n == 0:
        return res
    res["trials"][0] = lm_optimize(M, 5)
    c12, c21 = M.chi2()                                   # the stored errors: those of the last evaluated state
    bad = (c12 > th2) | (c21 > th2)
    cls = _classes_under_perturbation(M, M.S_eval, th2)
    res["decisive1"] = (cls == cls[0]).all(0)
    n_und = int((~res["decisive1"]).sum())
    n_bad = int(bad.sum())
    # every pair decisive; then nBad is exact, and nBad > 0 and nCorrespondences - nBad < 10 with it (written
    # out all the same: the count may move by at most n_und)
    nbad_gt0_sure = n_bad - n_und > 0 or n_bad + n_und == 0
    left = n - n_bad
    exit_sure = left + n_und < 10 or left - n_und >= 10
    res["decisive"] = bool(n_und == 0 and nbad_gt0_sure and exit_sure)
    res.update(n_bad=n_bad, inlier=~bad, chi2_12=c12.copy(), chi2_21=c21.copy())
    M.bad = bad
    M.robust = False
    if n - n_bad < 10:
        return res
    res["early"] = False
    res["trials"][1] = lm_optimize(M, 10 if n_bad > 0 else 5)
    a = ~bad
    e12, e21 = M.edge_errors(M.S)
    M.e12[a], M.e21[a] = e12[a], e21[a]
    c12, c21 = M.chi2()
    out2 = (c12 > th2) | (c21 > th2)
    cls = _classes_under_perturbation(M, M.S, th2)
    res["decisive2"] = (cls == cls[0]).all(0) | bad       # (a pair culled before is not judged again)
    inl = a & ~out2
    res.update(s12=M.S.vector(), n_in=int(inl.sum()), inlier=inl, chi2_12=c12, chi2_21=c21)
    return res


# ---- the host build of the kernel's arithmetic ----------------------------------------------------------------
def host_lib():
    """csrc/orb_optsim3_math.h compiled for the host (tests/native/optsim3_host.cpp) as a ctypes library."""
    import ctypes
    import pathlib
    import subprocess
    root = pathlib.Path(__file__).resolve().parents[1]
    build = root / "build" / "tests"
    build.mkdir(parents=True, exist_ok=True)
    so = build / "liboptsim3_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Werror",
                    str(root / "tests" / "native" / "optsim3_host.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.optsim3_host_exp.argtypes = [vp, vp]
    lib.optsim3_host_errors.argtypes = [vp, vp, vp, vp, vp]
    lib.optsim3_host_jacobian.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    lib.optsim3_host_solve.argtypes = [ci] + [vp] * 9 + [cf, ci] + [vp] * 6
    for f in (lib.optsim3_host_exp, lib.optsim3_host_errors, lib.optsim3_host_jacobian, lib.optsim3_host_solve):
        f.restype = None
    return lib


def _pairs(prob):
    """The 88-byte pair records the kernel keeps in LDS."""
    dt = np.dtype([("p1", "<f8", 3), ("p2", "<f8", 3), ("o1", "<f8", 2), ("o2", "<f8", 2), ("is1", "<f4"), ("is2", "<f4")])
    assert dt.itemsize == 88
    P = np.zeros(len(prob["p1c"]), dt)
    P["p1"], P["p2"], P["o1"], P["o2"] = prob["p1c"], prob["p2c"], prob["obs1"], prob["obs2"]
    P["is1"], P["is2"] = prob["inv_sigma2_1"], prob["inv_sigma2_2"]
    return P


def host_solve(prob, lib=None):
    """The whole schedule on the host build: the same dict entries as optimize_sim3 reports to the ABI."""
    lib = lib or host_lib()
    c = lambda a, d: np.ascontiguousarray(a, d)  # noqa: E731
    arrs = [c(prob[k], np.float64) for k in ("p1c", "p2c", "obs1", "obs2")] + \
        [c(prob[k], f32) for k in ("inv_sigma2_1", "inv_sigma2_2", "cam1", "cam2")] + [c(prob["s12"], np.float64)]
    n = len(arrs[0])
    s12, nn = np.zeros(8), np.zeros(2, np.int32)
    inl, c12, c21 = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1)), np.zeros(max(n, 1))
    trials = np.zeros(2, np.int32)
    lib.optsim3_host_solve(n, *[a.ctypes.data for a in arrs], float(prob["th2"]), int(prob["fix_scale"]), s12.ctypes.data,
                           nn.ctypes.data, inl.ctypes.data, c12.ctypes.data, c21.ctypes.data, trials.ctypes.data)
    return {"s12": s12, "n_in": int(nn[0]), "n_bad": int(nn[1]), "inlier": inl[:n].astype(bool), "chi2_12": c12[:n],
            "chi2_21": c21[:n], "trials": trials.tolist()}
