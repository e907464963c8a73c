"""Radar ingest of the fusion decoder -- host side, as in the reference, which
runs it in numpy on the main thread inside ``Detr3DHead.forward``
(HEAD:301-536).  The reference pulls the sweeps from the nuScenes devkit by
``sample_idx``; here the same raw arrays arrive through
``img_metas[i]['radar']``, produced by the data
pipeline:

    radar = dict(points={chan: [18,n] float64}, times={chan: [1,n]},
                 radar_rot={chan: wxyz}, lidar_rot=wxyz)

or an already-built ``[n,36]`` feature array.  The 36-column layout is the
contract of ``radar_feat_encoder`` (HEAD:183, 499-510).  The three module
constants POINT_RANGE, NUM_RADAR_TOKENS and NUM_FEATURES are the reference's and
the defaults of ``Detr3DHead(radar_point_range=, radar_num_tokens=,
radar_in_dims=)``; a head with another feature count takes ``[n,F]`` rows only.
"""
import numpy as np

RADAR_CHANNELS = ('RADAR_FRONT', 'RADAR_FRONT_LEFT', 'RADAR_FRONT_RIGHT',
                  'RADAR_BACK_LEFT', 'RADAR_BACK_RIGHT')
POINT_RANGE = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)      # HEAD:304
NUM_RADAR_TOKENS = 1500                                   # HEAD:526
PAD_VALUE = 500.0                                         # HEAD:527
#: raw-row columns copied verbatim: x y z id rcs is_quality_valid invalid_state
BASE_COLUMNS = (0, 1, 2, 4, 5, 10, 14)                    # HEAD:499
NUM_FEATURES = 36


def quaternion_rotation_matrix(q):
    """Rotation matrix of a (w, x, y, z) quaternion (pyquaternion semantics:
    the quaternion is normalised first)."""
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([
        [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
        [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _one_hot(idx, width):
    out = np.zeros((idx.shape[0], width))
    out[np.arange(idx.shape[0]), idx] = 1.0
    return out


def _channel_features(points, times, rot_radar, rot_ref):
    n = points.shape[1]

    def to_lidar(v_xy):                                   # HEAD:317-327
        v = np.vstack((v_xy, np.zeros(n)))
        v = rot_ref.T @ (rot_radar @ v)
        v[2, :] = 0.0
        return v.T[:, :2]
    v_comp = to_lidar(points[8:10, :])
    v_raw = to_lidar(points[6:8, :])
    rows = points.T
    if times.shape[1] != 0:                               # HEAD:453-455
        times = times - np.max(times)
    t2 = np.repeat(times.T, 2, axis=1)
    return np.concatenate(
        (rows[:, list(BASE_COLUMNS)], t2, v_comp * t2, v_comp, v_raw,
         _one_hot(rows[:, 3].astype(int), 8),             # dyn_prop
         _one_hot(rows[:, 11].astype(int), 5),            # ambig_state
         _one_hot(rows[:, 15].astype(int), 8)), axis=1)   # pdh0


def build_radar_features(radar, point_range=POINT_RANGE, num_features=NUM_FEATURES):
    """Raw multi-sweep radar of one sample -> [n_kept, 36] float64.  An ``[n, num_features]`` array is a frame whose rows
    the producer built (and filtered) itself: returned as it is.  The raw route exists for the 36 features of the
    reference alone."""
    if isinstance(radar, np.ndarray):
        if radar.ndim != 2 or radar.shape[1] != num_features:
            raise ValueError('radar feature rows of shape %s: [n, %d] expected (radar_in_dims=%d)'
                             % (radar.shape, num_features, num_features))
        return radar
    if num_features != NUM_FEATURES:
        raise ValueError('raw radar sweeps give the %d features of the reference; a head with radar_in_dims=%d takes '
                         '[n, %d] feature rows' % (NUM_FEATURES, num_features, num_features))
    rot_ref = quaternion_rotation_matrix(radar['lidar_rot'])
    per_chan = []
    for chan in RADAR_CHANNELS:
        pts = np.asarray(radar['points'][chan], dtype=np.float64)
        tms = np.asarray(radar['times'][chan], dtype=np.float64)
        per_chan.append(_channel_features(
            pts, tms, quaternion_rotation_matrix(radar['radar_rot'][chan]),
            rot_ref))
    allp = np.concatenate(per_chan, axis=0)
    lo, hi = np.asarray(point_range[:3]), np.asarray(point_range[3:])
    keep = np.all(allp[:, :3] > lo, axis=1) & np.all(allp[:, :3] < hi, axis=1)
    return allp[keep]


def in_range(rows, point_range):
    """HEAD:514-519 on rows [n, >= 3]: x, y, z strictly inside the range (float64; a NaN fails) -> bool [n]."""
    xyz = np.asarray(rows)[:, :3].astype(np.float64)
    return np.all(xyz > np.asarray(point_range[:3]), axis=1) & np.all(xyz < np.asarray(point_range[3:]), axis=1)


def pack_tokens(feature_list, granule=64, T=None, num_tokens=NUM_RADAR_TOKENS):
    """Batch of [n_i,F] arrays -> (tokens [B,T,F] float32, pad_mult).

    T: fixed token count (a frame pipeline's static ``tokens`` tensor has one
    shape for every frame: T and pad_mult are baked into its captured graph);
    None picks the smallest multiple of ``granule`` that holds the frame.
    num_tokens: the head's token count N (Detr3DHead.radar_num_tokens).

    The reference always attends over N = 1500 tokens, the unused ones filled
    with 500.0 (HEAD:526-530); a frame's points beyond the first N are dropped
    (HEAD:528).  Identical pad tokens have identical keys and values, so only
    T = round_up(max n_i + 1, granule) tokens are materialised and the last one
    carries the multiplicity of the missing N - T pad tokens (see
    tc_radar_gated_xattn_fwd); a frame that fills all N tokens has no pad row
    (T = N, pad_mult = 1)."""
    N = int(num_tokens)
    n_max = max(min(f.shape[0], N) for f in feature_list)
    widths = {f.shape[1] for f in feature_list}
    if len(widths) != 1:
        raise ValueError('radar feature rows of different widths in one batch: %s' % sorted(widths))
    if T is None:
        T = min(N, ((n_max + 1 + granule - 1) // granule) * granule)
    elif not (1 <= T <= N) or (n_max + 1 > T and T < N):
        raise ValueError('T=%d cannot hold %d radar points + one pad token (max %d)'
                         % (T, n_max, N))
    tokens = np.full((len(feature_list), T, widths.pop()), PAD_VALUE,
                     dtype=np.float32)
    for b, f in enumerate(feature_list):
        n = min(f.shape[0], T)
        tokens[b, :n] = f[:n].astype(np.float32)
    return tokens, N - T + 1
