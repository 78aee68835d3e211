"""numpy restatement of be_a2c_adam (include/ballenv.h): the pinned Adam step over the six Policy
tensors and the device state, one f64 operation at a time, and the per-row fixed-point form the
re-pack shares with be_policy_load's pack kernel (policy_core.h).  Test infrastructure only."""
import numpy as np

PARAMS = ("fc1.weight", "fc1.bias", "action_head.weight", "action_head.bias", "value_head.weight",
          "value_head.bias")
QMAX = 8323072          # 127 * 2^16


def fresh_state(lr):
    return np.array([0.0, 1.0, 1.0, lr], dtype=np.float64)


def adam_step_ref(w, g, m, v, state, beta1, beta2, eps):
    """One step in place.  w, g, m, v: dicts of f32 arrays (g is read); state: f64 [t, b1^t, b2^t, lr]."""
    t, p1, p2, lr = (np.float64(x) for x in state)
    beta1, beta2, eps = np.float64(beta1), np.float64(beta2), np.float64(eps)
    p1n, p2n = p1 * beta1, p2 * beta2
    bc1 = np.float64(1.0) - p1n
    bc2s = np.sqrt(np.float64(1.0) - p2n)
    ss = lr / bc1
    omb1, omb2 = np.float64(1.0) - beta1, np.float64(1.0) - beta2
    for k in w:
        assert w[k].dtype == g[k].dtype == m[k].dtype == v[k].dtype == np.float32
        gd = g[k].astype(np.float64)
        m1 = (beta1 * m[k].astype(np.float64) + omb1 * gd).astype(np.float32)
        v1 = (beta2 * v[k].astype(np.float64) + (omb2 * gd) * gd).astype(np.float32)
        w1 = (w[k].astype(np.float64) -
              ss * (m1.astype(np.float64) / (np.sqrt(v1.astype(np.float64)) / bc2s + eps))).astype(np.float32)
        m[k][...], v[k][...], w[k][...] = m1, v1, w1
    state[:] = (t + 1.0, p1n, p2n, lr)


def pack_rows_ref(w1, b1):
    """The per-row step s (f64), the bias bq (i32) and the three int8 digit planes (d2, d1, d0) of
    q = clip(rint(w / s)) for fc1.weight (H, F) / fc1.bias (H) in f32."""
    w1, b1 = np.asarray(w1, np.float32), np.asarray(b1, np.float32)
    mx = np.maximum(np.abs(w1).max(axis=1), np.abs(b1) * np.float32(1.0 / 64.0)).astype(np.float32)
    s = np.where(mx > 0, (mx.astype(np.float64) / 8323072.0).astype(np.float32).astype(np.float64), 1.0)
    bq = np.rint(b1.astype(np.float64) / s).astype(np.int64).astype(np.int32)
    q = np.clip(np.rint(w1.astype(np.float64) / s[:, None]).astype(np.int64), -QMAX, QMAX)
    d0 = ((q + 128) & 255) - 128
    q1 = (q - d0) >> 8
    d1 = ((q1 + 128) & 255) - 128
    d2 = (q1 - d1) >> 8
    return s, bq, (d2, d1, d0), q
