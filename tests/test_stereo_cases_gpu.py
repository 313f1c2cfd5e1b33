"""The built stereo scenes (tests/stereo_cases.py) on the GPU: compute_stereo_matches and
compute_stereo_matches_batch_device equal the Python reference (tests/stereo_ref.py) bit for bit, per
keypoint, plus the kept count.  The reference runs on the oracle extractor's level planes; the package's
planes are first checked to be the same on the view region."""
from __future__ import annotations

import numpy as np
import pytest

import stereo_cases as cases
from stereo_ref import stereo_ref

pytestmark = pytest.mark.gpu

LEVELS = range(8)


def oracle_planes(oracle, image):
    ex = oracle.OracleExtractor(200, 1.2, 8, 20, 7)
    ex(image, (0, 0))
    return [ex.level_padded(l) for l in LEVELS], ex.params()


def assert_planes_agree(ex, planes, what, frame=0):
    for l in LEVELS:
        got = ex.level_padded(l, frame)
        assert got.shape == planes[l].shape, (what, l)
        assert np.array_equal(got[19:-19, 19:-19], planes[l][19:-19, 19:-19]), f"{what}: level {l} view differs"


def assert_same(name, label, g, idx, r, ur, dp, kept):
    for k, i in enumerate(idx):
        msg = (f"{name}/{label}: {g.names[i]} (reference: {r.reasons[k]}): uR {ur[k]!r} vs {r.u_right[k]!r}, "
               f"depth {dp[k]!r} vs {r.depth[k]!r}")
        assert ur[k].view(np.uint32) == r.u_right[k].view(np.uint32), msg
        assert dp[k].view(np.uint32) == r.depth[k].view(np.uint32), msg
    assert kept == r.kept, f"{name}/{label}: kept {kept} vs {r.kept}"


@pytest.fixture(scope="module")
def extractors(pkg):
    mk = lambda: pkg.ORBextractor(200, 1.2, 8, 20, 7, max_width=cases.S, max_height=cases.S, max_batch=4)
    return mk(), mk()


@pytest.mark.parametrize("name", list(cases.GROUPS))
def test_group(pkg, oracle, extractors, name):
    import torch
    g = cases.GROUPS[name]()
    exl, exr = extractors
    exl(g.left_image, None, (0, 0))
    exr(g.right_image, None, (0, 0))
    pl, p = oracle_planes(oracle, g.left_image)
    pr, _ = oracle_planes(oracle, g.right_image)
    assert_planes_agree(exl, pl, f"{name} left")
    assert_planes_agree(exr, pr, f"{name} right")
    runs = list(g.subsets.items()) if g.subsets else [("all", np.arange(len(g.kps_l)))]
    for label, idx in runs:
        r = stereo_ref(g.kps_l[idx], g.desc_l[idx], g.kps_r, g.desc_r, pl, pr, p["scale"], p["inv_scale"], g.bf, g.b)
        assert r.reasons == [g.expected_reasons[i] for i in idx], (name, label)
        ur, dp, kept = pkg.compute_stereo_matches(exl, exr, g.kps_l[idx], g.desc_l[idx], g.kps_r, g.desc_r, g.bf, g.b)
        assert_same(name, label, g, idx, r, ur, dp, kept)
    # the same calls as one batch on the device: one frame per run, over the frame-0 pyramids of a batch-of-n
    # extraction of the same image pair
    n = len(runs)
    for lo in range(0, n, 4):
        part = runs[lo:lo + 4]
        b = len(part)
        L = torch.from_numpy(np.stack([g.left_image] * b)).cuda()
        R = torch.from_numpy(np.stack([g.right_image] * b)).cuda()
        exl.extract_batch_device(L, (0, 0))
        exr.extract_batch_device(R, (0, 0))
        cap_l, cap_r = max(len(idx) for _, idx in part) + 3, len(g.kps_r) + 2
        kl = np.zeros((b, cap_l), cases.KEYPOINT_DTYPE)
        dl = np.zeros((b, cap_l, 32), np.uint8)
        kr = np.zeros((b, cap_r), cases.KEYPOINT_DTYPE)
        dr = np.zeros((b, cap_r, 32), np.uint8)
        cl, cr = np.zeros((b, 2), np.int32), np.zeros((b, 2), np.int32)
        for f, (_, idx) in enumerate(part):
            kl[f, :len(idx)], dl[f, :len(idx)] = g.kps_l[idx], g.desc_l[idx]
            kr[f, :len(g.kps_r)], dr[f, :len(g.kps_r)] = g.kps_r, g.desc_r
            cl[f, 0], cr[f, 0] = len(idx), len(g.kps_r)
        u, d, kept = run_batch(pkg, exl, exr, kl, dl, cl, kr, dr, cr, g.bf, g.b)
        for f, (label, idx) in enumerate(part):
            r = stereo_ref(g.kps_l[idx], g.desc_l[idx], g.kps_r, g.desc_r, pl, pr, p["scale"], p["inv_scale"], g.bf, g.b)
            assert_same(name, f"batch/{label}", g, idx, r, u[f, :len(idx)], d[f, :len(idx)], kept[f])


def run_batch(pkg, exl, exr, kl, dl, cl, kr, dr, cr, bf, b):
    """compute_stereo_matches_batch_device on hand-built [B, cap] arrays; the outputs start as garbage."""
    import torch
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()
    bsz, cap_l = kl.shape
    out_l = (dev(kl, np.float32).reshape(bsz, cap_l, 7), dev(dl, np.uint8), dev(cl, np.int32))
    out_r = (dev(kr, np.float32).reshape(bsz, kr.shape[1], 7), dev(dr, np.uint8), dev(cr, np.int32))
    out = (torch.full((bsz, cap_l), 7.5, dtype=torch.float32, device="cuda"),
           torch.full((bsz, cap_l), 7.5, dtype=torch.float32, device="cuda"),
           torch.full((bsz,), -7, dtype=torch.int32, device="cuda"))
    u, d, kept = pkg.compute_stereo_matches_batch_device(exl, exr, out_l, out_r, bf, b, out=out)
    torch.cuda.synchronize()
    return u.cpu().numpy(), d.cpu().numpy(), kept.cpu().numpy()


def test_batch(pkg, oracle, extractors):
    import torch
    g = cases.batch()
    counts_l, counts_r, cap_l, cap_r = g.counts
    exl, exr = extractors
    exl.extract_batch_device(torch.from_numpy(g.left_image).cuda(), (0, 0))
    exr.extract_batch_device(torch.from_numpy(g.right_image).cuda(), (0, 0))
    torch.cuda.synchronize()
    bsz = len(counts_l)
    kl = np.zeros((bsz, cap_l), cases.KEYPOINT_DTYPE)
    dl = np.zeros((bsz, cap_l, 32), np.uint8)
    kr = np.zeros((bsz, cap_r), cases.KEYPOINT_DTYPE)
    dr = np.zeros((bsz, cap_r, 32), np.uint8)
    cl, cr = np.zeros((bsz, 2), np.int32), np.zeros((bsz, 2), np.int32)
    refs = []
    for f in range(bsz):
        pl, p = oracle_planes(oracle, g.left_image[f])
        pr, _ = oracle_planes(oracle, g.right_image[f])
        assert_planes_agree(exl, pl, f"batch left frame {f}", f)
        assert_planes_agree(exr, pr, f"batch right frame {f}", f)
        kl[f, :counts_l[f]], dl[f, :counts_l[f]] = g.kps_l[f], g.desc_l[f]
        kr[f, :counts_r[f]], dr[f, :counts_r[f]] = g.kps_r[f], g.desc_r[f]
        cl[f, 0], cr[f, 0] = counts_l[f], counts_r[f]
        r = stereo_ref(g.kps_l[f], g.desc_l[f], g.kps_r[f], g.desc_r[f], pl, pr, p["scale"], p["inv_scale"], g.bf, g.b)
        assert r.reasons == g.expected_reasons[f], f
        refs.append(r)
    u, d, kept = run_batch(pkg, exl, exr, kl, dl, cl, kr, dr, cr, g.bf, g.b)
    for f, r in enumerate(refs):
        one = cases.Group(None, None, g.kps_l[f], None, None, None, g.bf, g.b, g.expected_reasons[f], g.names[f])
        n = counts_l[f]
        assert_same("batch", f"frame{f}", one, np.arange(n), r, u[f, :n], d[f, :n], kept[f])
    assert kept[1] == kept[2] == 0 and kept[3] == counts_l[3] > 0
