"""Hand-built scenes of the SearchByBoW(KeyFrame, KeyFrame) / loop BoW problem tests.  Nodes are independent of
each other in the search, so a search scene is a pair of keyframes whose nodes each hold one case: descriptors are a
node's base descriptor with chosen bits flipped, which fixes every Hamming distance exactly.

A side is a dict: keys_un (the cv::KeyPoint layout), descriptors [n, 32], feat_vec {node: [idx]}, ok [n] uint8,
mp_id [n] int32 (pool index, -1: NULL), obs_ok [n] uint8, level_sigma2.  tests/test_bow_kf_ref_cpu.py asserts that
each scene still contains what it is for.
"""
from __future__ import annotations

import numpy as np

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])
NLEVELS = 8
SCALE_FACTORS = (1.2 ** np.arange(NLEVELS)).astype(np.float32)
LEVEL_SIGMA2 = (SCALE_FACTORS * SCALE_FACTORS).astype(np.float32)
NNRATIO = 0.7
A1, A2 = 100.0, 90.0  # the default angles: difference 10 degrees, rotation bin 0


def flip(base, lo, hi):
    """base with bits [lo, hi) flipped: at Hamming distance hi - lo, and |S1 xor S2| from another flip of base."""
    bits = np.unpackbits(base)
    bits[lo:hi] ^= 1
    return np.packbits(bits)


class Side:
    def __init__(self):
        self.desc, self.angle, self.ok, self.octave, self.fv, self.tag = [], [], [], [], {}, []

    def add(self, node, desc, angle, ok=1, octave=None, tag=-1):
        i = len(self.desc)
        self.tag.append(tag)
        self.desc.append(np.asarray(desc, np.uint8))
        self.angle.append(angle)
        self.ok.append(ok)
        self.octave.append(i % 4 if octave is None else octave)
        if node is not None:
            self.fv.setdefault(node, []).append(i)
        return i

    def build(self, seed):
        n = len(self.desc)
        rng = np.random.default_rng(seed)
        k = np.zeros(n, KEYPOINT_DTYPE)
        k["x"], k["y"] = rng.uniform(20, 700, n), rng.uniform(20, 460, n)
        k["size"], k["angle"], k["octave"], k["class_id"] = 31.0, np.asarray(self.angle, np.float32), self.octave, -1
        return dict(keys_un=k, descriptors=np.asarray(self.desc, np.uint8).reshape(n, 32), feat_vec=dict(self.fv),
                    ok=np.asarray(self.ok, np.uint8), mp_id=np.full(n, -1, np.int32), obs_ok=np.ones(n, np.uint8),
                    level_sigma2=LEVEL_SIGMA2, tag=np.asarray(self.tag, np.int32))


def edge_pair(big: int = 70):
    """(kf1, kf2, case nodes): one case per node, see the comments; filler nodes put 30 clean matches into rotation
    bin 0 so that a single match in another bin is removed by the orientation check."""
    rng = np.random.default_rng(7)
    q = lambda: rng.integers(0, 256, 32, dtype=np.uint8)  # noqa: E731
    a, b = Side(), Side()
    nodes = {}
    for i in range(30):  # filler: distance 5 to the first, 60 to the second
        base = q()
        a.add(100 + i, base, A1)
        b.add(100 + i, flip(base, 0, 5), A2)
        b.add(100 + i, flip(base, 50, 110), A2)
    base = q()  # best distance exactly TH_LOW = 50, second 156: rejected here, accepted by the Frame form
    nodes["exact50"] = (10, a.add(10, base, A1))
    b.add(10, flip(base, 0, 50), A2)
    b.add(10, flip(base, 100, 256), A2)
    base = q()  # 49: accepted
    nodes["d49"] = (11, a.add(11, base, A1))
    b.add(11, flip(base, 0, 49), A2)
    base = q()  # two candidates at distance 20 (positions 1 and 3): best = second, the ratio test fails below 1
    nodes["tie"] = (12, a.add(12, base, A1))
    b.add(12, flip(base, 0, 90), A2)
    nodes["tie_first_idx2"] = b.add(12, flip(base, 0, 20), A2)
    b.add(12, flip(base, 100, 200), A2)
    b.add(12, flip(base, 20, 40), A2)
    base = q()  # the second KF1 feature's nearest candidate (distance 4) is claimed: it takes the one at 34
    g = b.add(13, base, A2)
    g2 = b.add(13, flip(base, 100, 130), A2)
    a.add(13, flip(base, 0, 3), A1)
    nodes["claimed_best"] = (13, a.add(13, flip(base, 3, 7), A1), g, g2)
    base = q()  # the first KF1 feature claims g in rotation bin 6 and is removed; the second (distance 7) stays empty
    b.add(20, base, A2)
    nodes["rot_removed"] = (20, a.add(20, flip(base, 0, 5), 270.0))
    nodes["rot_blocked"] = (20, a.add(20, flip(base, 5, 12), A1))
    base = q()  # the nearest KF2 feature (distance 0) has no usable map point: the one at 20 is taken
    b.add(14, base, A2, ok=0)
    nodes["ok2_masked"] = (14, a.add(14, base, A1), b.add(14, flip(base, 0, 20), A2))
    base = q()  # KF1 feature without a usable map point
    nodes["ok1_masked"] = (15, a.add(15, base, A1, ok=0))
    b.add(15, base, A2)
    a.add(30, q(), A1)  # a node on one side only, each way
    b.add(31, q(), A2)

    def crowd(node, n_a, n_b, copies_from):
        """A node with n_a / n_b features around one base (0..45 random flipped bits); the first KF1 features are
        near copies of the KF2 features from position copies_from on, two KF1 features per KF2 feature, so that
        bests and claims fall on those positions."""
        base = q()
        gs = []
        for _ in range(n_b):
            lo = int(rng.integers(0, 200))
            gs.append(flip(base, lo, lo + int(rng.integers(0, 46))))
            b.add(node, gs[-1], A2, ok=int(rng.random() > 0.1))
        for i in range(n_a):
            j = copies_from + i // 2
            if j < n_b:
                d = flip(gs[j], 250, 250 + int(rng.integers(0, 4)))
            else:
                lo = int(rng.integers(0, 200))
                d = flip(base, lo, lo + int(rng.integers(0, 46)))
            a.add(node, d, A1, ok=int(rng.random() > 0.1))

    crowd(40, 16, big, 60)        # 65+ KF2 features: the register path and the memory path beyond position 64
    crowd(41, big, 6, 0)          # 65+ KF1 features
    crowd(42, big, big + 3, 58)   # both
    a.add(None, q(), A1)          # features no node lists
    b.add(None, q(), A2)
    return a.build(1), b.build(2), nodes


def variant(side, **over):
    d = dict(side)
    d.update(over)
    return d


def random_pair(seed, n1=150, n2=160, n_nodes=12, frac_ok=0.8, base_seed=None):
    """Two keyframes observing shared base descriptors with 0..40 flipped bits, random nodes of ~12 features,
    random angles around a common rotation: claims, ratio failures and rotation rejects all occur.  base_seed: the
    bases of another call, so that its keyframes match this one's."""
    rng = np.random.default_rng(seed)
    bases = np.random.default_rng(seed if base_seed is None else base_seed).integers(0, 256, (n_nodes * 6, 32),
                                                                                     dtype=np.uint8)
    out = []
    for n in (n1, n2):
        s = Side()
        for _ in range(n):
            w = int(rng.integers(0, len(bases)))
            lo = int(rng.integers(0, 200))
            ang = (3.0 * w + rng.normal(0, 4) + (0 if len(out) == 0 else 40) + (180 if rng.random() < 0.08 else 0)) % 360
            s.add(w // 6, flip(bases[w], lo, lo + int(rng.integers(0, 41))), float(ang), ok=int(rng.random() < frac_ok),
                  tag=w)
        out.append(s.build(seed + len(out)))
    return out


def search_scenes():
    """name -> (kf1, [kf2, ...]): every pair of a scene shares kf1 (one batched call)."""
    a, b, _ = edge_pair()
    r = random_pair(31)
    r2 = random_pair(32, base_seed=31)
    empty_fv = variant(r2[1], feat_vec={})
    no_ok2 = variant(b, ok=np.zeros(len(b["ok"]), np.uint8))
    return {"edges": (a, [b]), "edges_batch": (a, [b, empty_fv, r[1], no_ok2]), "random": (r[0], [r[1], r2[1], r2[0]]),
            "empty_fv1": (variant(r[0], feat_vec={}), [r[1]]),
            "no_ok1": (variant(a, ok=np.zeros(len(a["ok"]), np.uint8)), [b, r[1]])}


def merge_scene():
    """The hand-written merge / gather scene: KF1 with 12 features, 3 candidates x up to 3 window keyframes, a pool
    of 20 points.  Returns a dict: kf1, kfs2 (flat, candidate after candidate), group, pair_ok, matches12 [P, 12],
    xyz, bad, Tcw1, Tcw2.  The cases (candidate 0 unless said): the same point through j0 at k=1 and j1 at k=5; two
    new points at k=2 (j0: 6, j1: 9: overwrite, both counted); a bad point (7 at k=3); the same point at the same
    k through j0 and j2 (8 at k=4); a slot dropped by ok1 (k=7), by the window keyframe's obs_ok (k=8) and by KF1's
    obs_ok (k=9); candidate 1 has a pair_ok = 0 pair that would add points; candidate 2 has no match at all."""
    rng = np.random.default_rng(11)
    n1, n2 = 12, 10

    def side(seed, octs):
        s = Side()
        for i in range(len(octs)):
            s.add(i % 3, rng.integers(0, 256, 32, dtype=np.uint8), 0.0, octave=octs[i])
        return s.build(seed)

    kf1 = side(0, [0, 1, 2, 3, 4, 0, 1, 2, 3, 5, 0, 1])
    kf1["mp_id"][:] = [0, 1, 2, 3, 4, 14, 15, 16, 17, 18, 19, -1]
    kf1["ok"][:] = 1
    kf1["ok"][[7, 11]] = 0
    kf1["obs_ok"][9] = 0
    kfs2 = [side(1 + p, [(p + i) % 5 for i in range(n2)]) for p in range(6)]
    m12 = np.full((6, n1), -1, np.int32)

    def put(p, k, idx2, mp):
        m12[p, k] = idx2
        kfs2[p]["mp_id"][idx2] = mp

    put(0, 1, 3, 5); put(0, 2, 0, 6); put(0, 3, 7, 7); put(0, 4, 9, 8)        # noqa: E702
    put(1, 5, 2, 5); put(1, 2, 4, 9); put(1, 6, 1, 10)                          # noqa: E702
    put(2, 4, 6, 8); put(2, 7, 0, 11); put(2, 8, 5, 12); put(2, 9, 8, 13)      # noqa: E702
    m12[2, 10] = 3                                                              # a feature without a map point
    kfs2[2]["obs_ok"][5] = 0
    put(3, 0, 1, 5); put(3, 6, 2, 6)                                            # noqa: E702 candidate 1, j0
    put(4, 1, 0, 12); put(4, 6, 3, 13)                                          # noqa: E702 candidate 1, j1: pair_ok 0
    xyz = np.stack([rng.uniform(-4, 4, 20), rng.uniform(-2, 2, 20), rng.uniform(2, 10, 20)], 1).astype(np.float32)
    bad = np.zeros(20, np.uint8)
    bad[7] = 1

    def pose(yaw, t):
        c, s = np.cos(yaw), np.sin(yaw)
        return np.concatenate([np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), np.asarray(t).reshape(3, 1)], 1).astype(np.float32)

    return dict(kf1=kf1, kfs2=kfs2, group=np.array([0, 3, 5, 6], np.int32), pair_ok=np.array([1, 1, 1, 1, 0, 1], np.uint8),
                matches12=m12, xyz=xyz, bad=bad, Tcw1=pose(0.1, [0.3, -0.1, 0.2]),
                Tcw2=np.stack([pose(-0.2, [1.0, 0.1, -0.3]), pose(0.4, [-0.5, 0.0, 0.6]), pose(0.0, [0, 0, 0])]))


def chain_scene():
    """The search feeding the merge: kf1 and 2 candidates x 2 window keyframes of random_pair(), sharing 72 descriptor
    bases.  A feature of base w observes pool point w in kf1 and point 72 + w = S(point w) in a window keyframe, S one
    similarity: true matches are consistent Sim3 correspondences (the solver finds inliers), window keyframes of a
    candidate share points (the merge meets repeats), 5 % of the points are bad and one window keyframe has obs_ok
    holes.  Returns the same dict as merge_scene() without matches12 (the search's output)."""
    rng = np.random.default_rng(5)
    kf1 = random_pair(41, frac_ok=0.9)[0]
    kfs2 = [random_pair(41 + p, frac_ok=0.9, base_seed=41)[1] for p in range(4)]
    W = 72
    X = np.stack([rng.uniform(-4, 4, W), rng.uniform(-2, 2, W), rng.uniform(2, 10, W)], 1)
    c, sn = np.cos(0.3), np.sin(0.3)
    S = 1.3 * np.array([[c, -sn, 0], [sn, c, 0], [0, 0, 1]])
    xyz = np.concatenate([X, X @ S.T + np.array([0.5, -0.2, 1.0])]).astype(np.float32)
    bad = (rng.random(2 * W) < 0.05).astype(np.uint8)
    kfs2[2]["obs_ok"][::7] = 0
    for k, off in [(kf1, 0)] + [(k, W) for k in kfs2]:  # ok = map point non-NULL and not bad
        k["mp_id"] = np.where(k["ok"] != 0, k["tag"] + off, -1).astype(np.int32)
        k["ok"] = ((k["mp_id"] >= 0) & (bad[np.maximum(k["mp_id"], 0)] == 0)).astype(np.uint8)
    m = merge_scene()
    return dict(kf1=kf1, kfs2=kfs2, group=np.array([0, 2, 4], np.int32), pair_ok=None, xyz=xyz, bad=bad, Tcw1=m["Tcw1"],
                Tcw2=m["Tcw2"][:2])


def expected_search(ref, kf1, kf2, check_ori, nnratio=NNRATIO, stats=None):
    return ref.search_by_bow_kf(kf1["descriptors"], kf1["keys_un"]["angle"], kf1["feat_vec"], kf1["ok"],
                                kf2["descriptors"], kf2["keys_un"]["angle"], kf2["feat_vec"], kf2["ok"], nnratio,
                                check_ori, stats)


def expected_problems(ref, sc, matches12, ok1="scene"):
    """merge + gather of every candidate of a merge scene dict on the given matches12 rows: a list of dicts with
    num_bow, matched_point, matched_pair and gather()'s fields."""
    kf1, out = sc["kf1"], []
    n1 = len(kf1["ok"])
    ok1 = kf1["ok"] if isinstance(ok1, str) else ok1
    for c in range(len(sc["group"]) - 1):
        ps = range(sc["group"][c], sc["group"][c + 1])
        rows = [matches12[p][:n1] for p in ps]
        ks = [sc["kfs2"][p] for p in ps]
        pok = None if sc["pair_ok"] is None else [sc["pair_ok"][p] for p in ps]
        nb, mpt, mpr = ref.merge(rows, [k["mp_id"] for k in ks], sc["bad"], pok, n1)
        g = ref.gather(mpt, mpr, rows, kf1["mp_id"], ok1, sc["bad"], sc["xyz"], kf1["keys_un"]["octave"],
                       kf1["level_sigma2"], [k["keys_un"]["octave"] for k in ks], [k["level_sigma2"] for k in ks],
                       sc["Tcw1"], sc["Tcw2"][c], kf1["obs_ok"], [k["obs_ok"] for k in ks])
        g.update(num_bow=nb, matched_point=mpt, matched_pair=mpr)
        out.append(g)
    return out


def keyframe(pkg, side):
    """A side as the package's KeyFrame (its has_mappoint = ok)."""
    return pkg.KeyFrame(keys_un=side["keys_un"], descriptors=side["descriptors"], Tcw=np.eye(4, dtype=np.float32)[:3],
                        camera=(458.654, 457.296, 367.215, 248.375), scale_factors=SCALE_FACTORS,
                        level_sigma2=side["level_sigma2"], has_mappoint=side["ok"], feat_vec=side["feat_vec"])
