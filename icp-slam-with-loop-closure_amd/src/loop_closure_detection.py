"""Drop-in ``src/loop_closure_detection.py``: loop-closure search with the ICP
alignments batched on MI355X.

Same functions and arguments as the reference module
(``/root/reference/src/loop_closure_detection.py``), which ``scripts/main.py``
imports at start-up (``scripts/main.py:19``).  The reference imports OpenCV at
module level; here only the image path needs it and imports it when called,
so the module (and ``scripts/main.py``) imports on a host without cv2.

* ``detect_proximity`` (reference :11-39): candidate pairs from the pose
  geometry (same cdist / path-length rule), then ONE batched ICP launch over
  every candidate (init identity, eps 0.05, max_iters 100) instead of one
  ``icp.icp`` call per accepted candidate; the reference's greedy pass (reverse
  order, each node used once, ``error < err_thresh``) is replayed on the batch
  results.  A pair's ICP result does not depend on the others, so the
  constraints added are the reference's; candidates the greedy pass skips are
  computed and discarded.
* ``detect_images_direct_similarity`` (reference :81-175): ORB keypoints and
  descriptor matching stay OpenCV's (ImportError without it); the ICP
  alignment of the accepted image matches (reference :136-142, a joblib
  fan-out) is one batched launch.

New, opt-in (a trailing keyword of both functions; the reference's call shapes
bind unchanged): ``init="csm"`` starts every ICP from the batched correlative
scan match of its pair (``slamhip.csm``; ``csm``: its ``CsmParams``) instead
of the identity, for loops closed at another heading.  The default
``init="identity"`` is the reference's behaviour.  ``detect_proximity`` also
takes ``candidates="device"``: the same candidate pairs from the GPU search of
``slamhip.lcd`` (O(N) memory) instead of the N x N ``cdist`` matrix of the
default ``candidates="host"``.  ``detect_images_direct_similarity`` takes
``matcher="device"``: the descriptor matching (``slamhip.desc``, brute force on
the GPU: ``approximate_match=True`` -> the exact ``l2`` search the FLANN kd-tree
approximates, ``False`` -> cross-checked ``hamming``), the selection and the ICP
run as ``slamhip.pipeline.image_loop_closures``; with ``descriptors=`` (one
(n, 32) uint8 array per image) OpenCV is not needed at all.  The default
``matcher="opencv"`` is the path above.

New function: ``detect_signatures`` proposes loop closures from the scans
themselves (rotation-invariant signatures matched on the GPU, ``slamhip.sig``),
needing neither nearly right poses nor a camera.

New, opt-in: ``detect_proximity`` and ``detect_signatures`` take ``verify=`` (a
``slamhip.vis.VisParams``): a candidate below its error threshold is added only
if its transform also passes the per-edge visibility check on the GPU; they
then return the number of candidates the check rejected.

New function: ``filter_consistent`` checks the loop closures the detectors
added against each other and removes those outside the pairwise consistent set
(``slamhip.pcm``, on the GPU), before the optimisation sees them.
"""
import numpy as np
import scipy.spatial

from slamhip import icp as _k
from slamhip.pipeline import add_loop_constraint, check_loop_closure_init, loop_closure_inits


def _cv2():
    try:
        import cv2
    except ImportError as e:   # image loop closures need OpenCV, like the reference
        raise ImportError("image-based loop closure detection needs OpenCV (cv2); "
                          "detect_proximity does not") from e
    return cv2


def _homog(p):
    p = np.asarray(p, dtype=np.float64)
    return np.c_[p[:, :2], np.ones(len(p))]


def _icp_pairs(pc1_list, pc2_list, init, csm, verify=None, err_thresh=None):
    """``slamhip.icp.icp_pairs`` (eps 0.05, max_iters 100) over one ScanSet
    that the opt-in correlative scan match of the same pairs shares.  With
    ``verify`` (a ``slamhip.vis.VisParams``): (result, the
    ``slamhip.pipeline.ClosureCheck`` of the pairs below ``err_thresh``)."""
    scans = [s for pair in zip(pc1_list, pc2_list) for s in pair]
    B = len(pc1_list)
    src, dst = np.arange(0, 2 * B, 2), np.arange(1, 2 * B, 2)
    ss = _k.ScanSet(scans)
    res = _k.icp_batch(ss, src, dst, loop_closure_inits(ss, src, dst, init, csm), epsilon=0.05, max_iters=100)
    if verify is None:
        return res
    from slamhip.pipeline import verify_closures
    return res, verify_closures(ss, src, dst, res.tf, res.err < err_thresh, verify)


def _path_geometry(poses):
    d = scipy.spatial.distance.cdist(poses[:, :2], poses[:, :2])
    walked = np.append([0], np.cumsum(np.diag(d, k=1)))
    return d, walked


def proximity_candidates(poses, min_dist_along_path=2, max_dist=1):
    """(i, j) pairs of reference :12-24, in the order the greedy pass visits them."""
    d, walked = _path_geometry(poses)
    out = []
    for i in range(len(poses)):
        s = np.searchsorted(walked, walked[i] + min_dist_along_path, side="right")
        if s >= len(poses):
            break
        j = s + int(np.argmin(d[i, s:]))
        if d[i, j] <= max_dist:
            out.append((i, j))
    out.reverse()
    return out


def detect_proximity(pose_graph, lidar_points, min_dist_along_path=2, max_dist=1, err_thresh=110,
                     init="identity", csm=None, candidates="host", verify=None):
    """``verify`` (a ``slamhip.vis.VisParams``; new, opt-in, the default None is
    the reference's behaviour): a candidate below ``err_thresh`` is added only
    if its transform also passes the visibility check (``slamhip.vis``); the
    greedy pass sees only those.  Returns None, or with ``verify`` the number of
    candidates the check rejected."""
    check_loop_closure_init(init)
    if candidates == "host":
        cand = proximity_candidates(pose_graph.poses, min_dist_along_path, max_dist)
    elif candidates == "device":
        from slamhip.lcd import proximity_candidates_device
        cand = proximity_candidates_device(pose_graph.poses, min_dist_along_path, max_dist)
    else:
        raise ValueError(f"unknown candidate search {candidates!r} (host | device)")
    if not cand:
        return None if verify is None else 0
    # icp(pc_j, pc_i) for every candidate, one launch (reference :33-35)
    res = _icp_pairs([_homog(lidar_points[j]) for _, j in cand], [_homog(lidar_points[i]) for i, _ in cand],
                     init, csm, verify, err_thresh)
    report = None
    if verify is not None:
        res, report = res
    used = set()
    for b, (i, j) in enumerate(cand):
        if i in used or j in used:
            continue
        error = float(res.err[b])
        if error < err_thresh and (report is None or report.ok[b]):
            print("%d %d %f" % (i, j, error))
            # icp(pc_j, pc_i): X_j = X_i T, the "relative" convention (src/pose_graph.py)
            add_loop_constraint(pose_graph, i, j, res.tf[b].copy(), "relative")
            used.update((i, j))
    return None if report is None else report.rejected


def detect_signatures(pose_graph, lidar_points, min_dist_along_path=5, max_frac=(1, 4), err_thresh=110,
                      init="signature", csm=None, params=None, verify=None):
    """New, without a counterpart in the reference: loop closures from the scans
    alone, beside ``detect_proximity`` and with its shape.  Every scan's best
    rotation-invariant signature match at least ``min_dist_along_path`` further
    along the path (``slamhip.sig``, searched on the GPU; the poses are not
    asked for nearness), icp(pc_j, pc_i) of all of them in one launch from the
    rotation the match found, and the same greedy pass
    (``slamhip.pipeline.signature_loop_closures``).  For revisits in the
    direction of travel, at any rotation of the scan frame.  ``verify``: as in
    ``detect_proximity``."""
    from slamhip.pipeline import signature_loop_closures
    out = signature_loop_closures(pose_graph, lidar_points, min_dist_along_path, max_frac, err_thresh, init=init,
                                  csm=csm, params=params, verify=verify)
    return None if verify is None else out[2].rejected


def filter_consistent(pose_graph, params=None, remove=True):
    """New, without a counterpart in the reference: checks the loop closures
    the detectors above added against each other and removes those outside the
    pairwise consistent set (``slamhip.pipeline.verify_loop_closures``,
    ``slamhip.pcm``; on the GPU).  Call it before the optimisation.  Returns
    the edges (i, j, T), the mask of those kept and the number of constraint
    edges without a recorded convention, which stay unverified."""
    from slamhip.pipeline import verify_loop_closures
    return verify_loop_closures(pose_graph, params, remove)


def serialize_keypoints(kp, des):
    return [(p.pt, p.size, p.angle, p.response, p.octave, p.class_id, d) for p, d in zip(kp, des)]


def deserialize_keypoints(serialized_keypoints):
    cv2 = _cv2()
    kp = [cv2.KeyPoint(x=s[0][0], y=s[0][1], size=s[1], angle=s[2], response=s[3], octave=s[4], class_id=s[5])
          for s in serialized_keypoints]
    return kp, np.array([s[6] for s in serialized_keypoints])


def serialize_matches(matches):
    return [(m.queryIdx, m.trainIdx, m.distance) for m in matches]


def deserialize_matches(serialized_matches):
    cv2 = _cv2()
    return [cv2.DMatch(s[0], s[1], s[2]) for s in serialized_matches]


def find_keypoints(img):
    kp, des = _cv2().ORB_create().detectAndCompute(img, None)
    return serialize_keypoints(kp, des)


def matchify(desc1, desc2, i, j, n_matches, approximate_match):
    cv2 = _cv2()
    if approximate_match:
        flann = cv2.FlannBasedMatcher(dict(algorithm=0, trees=5), dict(checks=50))
        matches = flann.match(np.asarray(desc1, np.float32), np.asarray(desc2, np.float32))
    else:
        matches = cv2.BFMatcher(cv2.NORM_HAMMING, crossCheck=True).match(desc1, desc2)
    matches = sorted(matches, key=lambda m: m.distance)
    if len(matches) < n_matches:
        return np.inf
    best = matches[:n_matches]
    return np.sum([m.distance for m in best]), serialize_matches(best), (i, j)


def detect_images_direct_similarity(pose_graph, lidar_points, images, image_rate=1, min_dist_along_path=5,
                                    image_err_thresh=125, n_matches=10, icp_err_thresh=30, save_dists=False,
                                    save_matches=False, n_jobs=-1, approximate_match=True,
                                    init="identity", csm=None, matcher="opencv", descriptors=None):
    check_loop_closure_init(init)
    if matcher == "device":
        return _detect_images_device(pose_graph, lidar_points, images, image_rate, min_dist_along_path,
                                     image_err_thresh, n_matches, icp_err_thresh, save_dists, save_matches, n_jobs,
                                     approximate_match, init, csm, descriptors)
    if matcher != "opencv":
        raise ValueError(f"unknown matcher {matcher!r} (opencv | device)")
    cv2 = _cv2()
    from joblib import Parallel, delayed
    d, walked = _path_geometry(pose_graph.poses)
    start = np.array([np.searchsorted(walked, w + min_dist_along_path, side="right") for w in walked])
    start[start == len(start)] = start[start == len(start)] * image_rate
    start = np.floor(start[::image_rate] / image_rate).astype(int)

    greys = [cv2.cvtColor(np.asarray(im, dtype=np.uint8), cv2.COLOR_RGB2GRAY) for im in images]
    par = Parallel(n_jobs=n_jobs, verbose=0, backend="loky")
    kps = par(delayed(find_keypoints)(greys[i]) for i in range(0, len(greys), image_rate))
    keypoints, descriptors = zip(*[deserialize_keypoints(s) for s in kps])
    scored = par(delayed(matchify)(descriptors[i], descriptors[j], i, j, n_matches, approximate_match)
                 for i in range(len(descriptors)) for j in range(start[i], len(descriptors)))
    dist_mat = np.full((len(descriptors), len(descriptors)), np.inf)
    matched = {}
    for r in scored:
        if np.isscalar(r):   # fewer than n_matches matches
            continue
        dist, ser, (i, j) = r
        dist_mat[i, j] = dist
        matched[(i, j)] = deserialize_matches(ser)
    print("Closest images keypoint match error %f" % np.min(dist_mat))
    if save_dists:
        import matplotlib.pyplot as plt
        for img, name in ((dist_mat, "dist_mat"), (dist_mat < image_err_thresh, "dist_mat_threshed")):
            fig, ax = plt.subplots()
            ax.imshow(img)
            plt.savefig("results/%s.png" % name)
            plt.close(fig)
    good = []
    for j in range(dist_mat.shape[1]):
        i = int(np.argmin(dist_mat[:, j]))
        if dist_mat[i, j] < image_err_thresh:
            good.append((i, j))
    if not good:
        return
    # reference :136-142: icp(pc_i, pc_j, init eye, max_iters 100, eps 0.05) per match -> one launch
    res = _icp_pairs([_homog(lidar_points[i * image_rate]) for i, _ in good],
                     [_homog(lidar_points[j * image_rate]) for _, j in good], init, csm)
    for b, (i0, j0) in enumerate(good):
        i, j = i0 * image_rate, j0 * image_rate
        if float(res.err[b]) < icp_err_thresh:
            add_loop_constraint(pose_graph, i, j, res.tf[b].copy(), "icp")   # icp(pc_i, pc_j): X_i = X_j T
            if save_matches:
                img = cv2.drawMatches(greys[i], keypoints[i0], greys[j], keypoints[j0], matched.get((i0, j0), []), None,
                                      flags=cv2.DrawMatchesFlags_NOT_DRAW_SINGLE_POINTS)
                cv2.imwrite("results/match_%d_%d_%f.png" % (i, j, dist_mat[i0, j0]), img)


def _save_dist_images(dist_mat, image_err_thresh):
    import matplotlib.pyplot as plt
    for img, name in ((dist_mat, "dist_mat"), (dist_mat < image_err_thresh, "dist_mat_threshed")):
        fig, ax = plt.subplots()
        ax.imshow(img)
        plt.savefig("results/%s.png" % name)
        plt.close(fig)


def _detect_images_device(pose_graph, lidar_points, images, image_rate, min_dist_along_path, image_err_thresh,
                          n_matches, icp_err_thresh, save_dists, save_matches, n_jobs, approximate_match, init, csm,
                          descriptors):
    """``matcher="device"``: the matching, the selection and the ICP of
    ``slamhip.pipeline.image_loop_closures``.  With ``descriptors`` (one
    (n, 32) uint8 array per image, image m of scan m * image_rate) OpenCV is
    never imported; without them the ORB keypoints still come from it."""
    from slamhip import desc as _desc
    from slamhip.pipeline import image_stage
    metric = "l2" if approximate_match else "hamming"
    greys = keypoints = None
    if descriptors is None:
        cv2 = _cv2()
        from joblib import Parallel, delayed
        greys = [cv2.cvtColor(np.asarray(im, dtype=np.uint8), cv2.COLOR_RGB2GRAY) for im in images]
        par = Parallel(n_jobs=n_jobs, verbose=0, backend="loky")
        kps = par(delayed(find_keypoints)(greys[i]) for i in range(0, len(greys), image_rate))
        keypoints, descriptors = zip(*[deserialize_keypoints(s) for s in kps])
    elif save_matches:
        raise ValueError("save_matches=True draws OpenCV keypoints: not available with descriptors= "
                         "(pass save_matches=False, or images without descriptors)")
    ds = descriptors if isinstance(descriptors, _desc.DescriptorSet) else _desc.DescriptorSet(descriptors)
    good, accepted, dist_mat, _ = image_stage(pose_graph, lidar_points, ds, image_rate, min_dist_along_path,
                                              image_err_thresh, n_matches, icp_err_thresh, metric, None, init, csm)
    print("Closest images keypoint match error %f" % (np.min(dist_mat) if dist_mat.size else np.inf))
    if save_dists:
        _save_dist_images(dist_mat, image_err_thresh)
    if save_matches and accepted.any():
        cv2 = _cv2()
        drawn = [g for g, ok in zip(good, accepted) if ok]
        rows = _desc.match_pairs(ds, [i for i, _ in drawn], [j for _, j in drawn], n_matches, metric,
                                 return_matches=True)[2]
        for (i0, j0), m in zip(drawn, rows):
            i, j = i0 * image_rate, j0 * image_rate
            dm = [cv2.DMatch(int(a), int(b), float(np.sqrt(np.float32(d))) if approximate_match else float(d))
                  for a, b, d in m]
            img = cv2.drawMatches(greys[i], keypoints[i0], greys[j], keypoints[j0], dm, None,
                                  flags=cv2.DrawMatchesFlags_NOT_DRAW_SINGLE_POINTS)
            cv2.imwrite("results/match_%d_%d_%f.png" % (i, j, dist_mat[i0, j0]), img)
