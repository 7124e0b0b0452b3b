"""numpy float32 restatements shared by the TrackEnv tests: the waypoint table, the 40-column rows and their adjoint (true IEEE
divisions, the summation order include/visfly_amd.h states)"""
import numpy as np

F = np.float32


def waypoints_np(n=10, center=(2, 0, 1), radius=2, radius_spd=0.2 * np.pi, dt=0.1):
    """TrackEnv.update_target at t == 0 (envs/TrackingEnv.py:74-79): ts and the argument in float32, cos / sin as the fp64 result rounded
    once, then radius * c + center in float32"""
    ts = np.arange(n).astype(np.float32) * F(dt)
    arg = F(radius_spd) * ts
    c, s = np.cos(arg.astype(np.float64)).astype(np.float32), np.sin(arg.astype(np.float64)).astype(np.float32)
    return np.stack([F(radius) * c + F(center[0]), F(radius) * s + F(center[1]), F(0) * s + F(center[2])], axis=1).astype(np.float32)


def track_rows_np(raw, wp, radius=10.0):
    """(N, 13) raw state rows -> (N, 3 P + 10): [(wp[j] - p) / R, q, v / 10, w / 10]"""
    raw, wp = np.asarray(raw, np.float32), np.asarray(wp, np.float32)
    rel = (wp[None, :, :] - raw[:, None, 0:3]).reshape(raw.shape[0], -1) / F(radius)
    return np.hstack([rel, raw[:, 3:7], raw[:, 7:10] / F(10), raw[:, 10:13] / F(10)]).astype(np.float32)


def track_rows_bwd_np(d, P, radius=10.0):
    """(N, 3 P + 10) -> (N, 13): dp[c] = -(sum_j d[3 j + c] / R), each term divided first, added in the order j = 0, 1, .."""
    d = np.asarray(d, np.float32)
    acc = d[:, 0:3] / F(radius)
    for j in range(1, P):
        acc = acc + d[:, 3 * j:3 * j + 3] / F(radius)
    return np.hstack([-acc, d[:, 3 * P:3 * P + 4], d[:, 3 * P + 4:3 * P + 7] / F(10), d[:, 3 * P + 7:3 * P + 10] / F(10)]).astype(np.float32)
