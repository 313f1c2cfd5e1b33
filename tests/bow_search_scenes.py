"""Scene helpers of the SearchByBoW / TrackReferenceKeyFrame GPU tests: keyframe variants, FeatureVector
remaps that merge nodes, and the staging of a host keyframe as a DeviceKeyFrame (the
orb_extract_batch_device / orb_bow_transform_frames_device layout with capacity past the count)."""
from __future__ import annotations

import numpy as np


def variant(pkg, k, **over):
    d = dict(keys_un=k.mvKeysUn, descriptors=k.mDescriptors, Tcw=k.Tcw, camera=(k.fx, k.fy, k.cx, k.cy),
             scale_factors=k.mvScaleFactors, level_sigma2=k.mvLevelSigma2, u_right=k.mvuRight,
             has_mappoint=k.has_mappoint, feat_vec=k.mFeatVec)
    d.update(over)
    return pkg.KeyFrame(**d)


def merge_nodes(feat_vec: dict, fn) -> dict:
    """node -> fn(node), each merged node's feature indices ascending (as DBoW2 fills a FeatureVector)."""
    out: dict = {}
    for node, idx in feat_vec.items():
        out.setdefault(fn(node), []).extend(idx)
    return {k: sorted(v) for k, v in out.items()}


def device_keyframe(pkg, K, cap: int, has_mappoint=None, count=None, n_nodes=None):
    """K (a pkg.KeyFrame) as frame 0 of device arrays of capacity `cap`: junk past the counts that a
    search must not read.  count / n_nodes override the device counts (a flagged side)."""
    import torch
    dev = torch.device("cuda")
    rng = np.random.default_rng(K.N + cap)
    pad = cap - K.N
    assert pad >= 0

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)

    src = K.mvKeysUn if K.N else np.zeros(1, K.mvKeysUn.dtype)
    k = np.concatenate([K.mvKeysUn, src[rng.integers(0, len(src), pad)]])
    k["angle"][K.N:] = rng.uniform(0, 360, pad)
    d = np.concatenate([K.mDescriptors, rng.integers(0, 256, (pad, 32), dtype=np.uint8)])
    nn = len(K.fv_node)
    fv_node = np.full(cap, 7, np.int32)
    fv_node[:nn] = K.fv_node.astype(np.int32)
    fv_begin = np.full(cap + 1, cap, np.int32)
    fv_begin[:nn + 1] = K.fv_offset
    fv_feat = rng.integers(0, cap, cap).astype(np.int32)
    fv_feat[:len(K.fv_index)] = K.fv_index
    hm = K.has_mappoint if has_mappoint is None else has_mappoint
    hmt = None
    if hm is not None:
        hmt = up(np.concatenate([np.asarray(hm, np.uint8), np.ones(pad, np.uint8)]).reshape(1, cap), np.uint8)
    extracted = (up(k.view(np.float32).reshape(1, cap, 7), np.float32), up(d.reshape(1, cap, 32), np.uint8),
                 up(np.array([[K.N if count is None else count, 0]]), np.int32))
    bow = (None, None, up(fv_node.reshape(1, cap), np.int32), up(fv_begin.reshape(1, cap + 1), np.int32),
           up(fv_feat.reshape(1, cap), np.int32), up(np.array([[0, nn if n_nodes is None else n_nodes]]), np.int32))
    return pkg.DeviceKeyFrame(extracted, bow, 0, K.Tcw, (K.fx, K.fy, K.cx, K.cy), K.mvScaleFactors, K.mvLevelSigma2,
                              has_mappoint=hmt)
