"""The objective value restated in numpy (csrc/cost_eval.hpp's comment, operation by operation): loops over i and j in Python, vectorised
over instances only, so every product, difference and sum is one rounding and every sum runs in the header's order.  Shared by
tests/test_cost_eval.py (against the header on the CPU) and tests/test_gpu_cost.py (against the kernels)."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def q_of(V, W, z, yref):
    """V [ny][nz], W [ny][ny], z [B][nz], yref [B][ny] -> q [B]"""
    ny, nz = V.shape
    B = z.shape[0]
    r = []
    for i in range(ny):
        y = np.zeros(B)
        for j in range(nz):
            y = y + V[i, j] * z[:, j]
        r.append(y - yref[:, i])
    q = np.zeros(B)
    for i in range(ny):
        t = np.zeros(B)
        for j in range(ny):
            t = t + W[i, j] * r[j]
        q = q + r[i] * t
    return q


def stage(tab, dt, u, x, yref, sl, su):
    """c_k, ls_k, slack_k [B] of one stage k < N: u [B][nu], x [B][nx], yref [B][ny], sl / su [B][>= K]; tab["K"] rows enter (0: hard rows)"""
    V = np.concatenate([tab["Vu"], tab["Vx"]], axis=1)
    ls = (0.5 * dt) * q_of(V, tab["W"], np.concatenate([u, x], axis=1), yref)
    S = np.zeros(x.shape[0])
    for i in range(tab["K"]):
        S = S + (((tab["zl"][i] * sl[:, i] + tab["zu"][i] * su[:, i]) + (0.5 * tab["Zl"][i]) * (sl[:, i] * sl[:, i]))
                 + (0.5 * tab["Zu"][i]) * (su[:, i] * su[:, i]))
    slack = dt * S
    return ls + slack, ls, slack


def evaluate(tab, dt, x, u, yref, yref_e, sl, su):
    """x [B][N+1][nx], u [B][N][nu], yref [B][N][ny], yref_e [B][ny_e], sl / su [B][N][K] -> c [B][N+1], cost [B], parts [B][3]"""
    B, N = u.shape[0], u.shape[1]
    c = np.zeros((B, N + 1))
    cost, p_ls, p_slack = np.zeros(B), np.zeros(B), np.zeros(B)
    for k in range(N):
        c[:, k], ls, slack = stage(tab, dt, u[:, k], x[:, k], yref[:, k], sl[:, k], su[:, k])
        cost = cost + c[:, k]
        p_ls = p_ls + ls
        p_slack = p_slack + slack
    c[:, N] = 0.5 * q_of(tab["Vx_e"], tab["W_e"], x[:, N], yref_e)
    cost = cost + c[:, N]
    return c, cost, np.stack([p_ls, c[:, N], p_slack], axis=1)


def tab_of_ocp(ocp, K, soft):
    """the tables of an AcadosOcp as the library reads them; K obstacle rows whose slacks enter the cost only when they are soft"""
    co = ocp.cost
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    Ks = K if soft else 0
    pen = {k: f(getattr(co, k)).reshape(-1)[:Ks] if Ks else np.zeros(0) for k in ("zl", "zu", "Zl", "Zu")}
    return dict(Vu=f(co.Vu), Vx=f(co.Vx), W=f(co.W), Vx_e=f(co.Vx_e), W_e=f(co.W_e), K=Ks, **pen)
