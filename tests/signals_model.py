"""A numpy model of the signals of the device step (include/ftgp.h: ftgp_device_io_signals / ftgp_step_device_ex), written from the
header's specification alone: the pooled scan and the state row.  tests/test_device_signals.py checks the model on hand-written rows
(CPU) and the library against it on the read-backs of a twin handle (GPU, tests/device_signals_child.py).

Every operation is one IEEE operation in the stated precision: numpy evaluates a * b + c * d as three array operations, never fused.
"""
import numpy as np

STATE_FLOATS = 8


def pool_scan(rows, pool, M):
    """rows float32 [..., n_rays] as ftgp_get_lidar lays them out -> float32 [..., n_rays / pool].
    M == 0: the minimum of the ranges >= 0 of a beam, -1 for a beam without one.  M > 0: every range r counts as r < 0 ? M : min(r, M),
    and the beam's minimum is multiplied by inv = float32(1) / float32(M)."""
    rows = np.asarray(rows, dtype=np.float32)
    pool = int(pool)
    assert pool >= 1 and rows.shape[-1] % pool == 0
    r = rows.reshape(rows.shape[:-1] + (rows.shape[-1] // pool, pool))
    if M == 0:
        m = np.where(r < 0, np.float32(np.inf), r).min(axis=-1)
        return np.where(np.isinf(m), np.float32(-1.0), m).astype(np.float32)
    M = np.float32(M)
    inv = np.float32(1.0) / M
    m = np.where(r < 0, M, np.minimum(r, M)).min(axis=-1).astype(np.float32)
    out = m * inv
    assert out.dtype == np.float32
    return out


def state_rows(pose, ctrl, progress, dist2):
    """float32 [n_cars, 8] from the host read-backs pose() [n, 13], ctrl() [n, 2], progress() [n, 10] and centre_dist2() [n]."""
    pose, ctrl, dist2 = (np.asarray(x, dtype=np.float64) for x in (pose, ctrl, dist2))
    progress = np.asarray(progress)
    qw, qz, vx, vy, wz = pose[:, 3], pose[:, 6], pose[:, 7], pose[:, 8], pose[:, 12]
    c = qw * qw - qz * qz
    s = 2.0 * (qw * qz)
    out = np.empty((len(pose), STATE_FLOATS), dtype=np.float32)
    out[:, 0] = vx * c + vy * s
    out[:, 1] = vy * c - vx * s
    out[:, 2] = wz
    out[:, 3] = ctrl[:, 0]
    out[:, 4] = ctrl[:, 1]
    out[:, 5] = np.sqrt(dist2)
    out[:, 6] = progress[:, 2].astype(np.float64) / 100.0
    out[:, 7] = progress[:, 5] != 0
    return out


def centre_dist2(pose, paths):
    """float64 [n_cars]: ((path - xy) ** 2).sum(1).min() per car (custom.py:1343, squared); paths [n_cars, 100, 2] = each car's centre-line."""
    pose = np.asarray(pose, dtype=np.float64)
    d = np.asarray(paths, dtype=np.float64) - pose[:, None, 0:2]
    return (d ** 2).sum(axis=2).min(axis=1)


def beam_classes(rows, pool, M):
    """(mixed, all_miss, clipped): beams that mix rays without a hit and hits, beams without any hit, ranges above M (0 when M == 0)."""
    rows = np.asarray(rows, dtype=np.float32)
    r = rows.reshape(rows.shape[:-1] + (rows.shape[-1] // int(pool), int(pool)))
    miss = r < 0
    mixed = int((miss.any(axis=-1) & ~miss.all(axis=-1)).sum())
    return mixed, int(miss.all(axis=-1).sum()), int((rows > M).sum()) if M > 0 else 0


def open_right_track():
    """The fixture map of the signals tests: 240 x 240 px over [-10, 10]^2, 3-px walls on the left, top and bottom edges, the right side
    open -- scans there hold hits, rays without a hit and ranges of up to 20 units, and nothing keeps a car on the centre-line circle."""
    from tests.walls_model import synthetic
    wall = np.zeros((240, 240), dtype=bool)
    wall[:, :3] = True
    wall[:3, :] = True
    wall[-3:, :] = True
    return synthetic(wall, 20.0 / 240, 20.0 / 240, -10.0, 10.0, "open-right")
