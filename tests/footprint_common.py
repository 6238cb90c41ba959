"""The footprint forward model restated in float64 (numpy and torch), what csrc/footprint.hip is checked against.

Sub-sample k of datum i is row i*K + k.  p_i = sum_k fw[k] y[i*K + k];  r = p - t;  loss = inv_count * sum_i wt_i r_i^2;
dL/dy[i*K + k] = fw[k] * 2 wt_i r_i inv_count, inv_count = 1 / (count_total or n).
"""
import numpy as np
import torch


def reduce64(y, fw):
    fw = np.asarray(fw, np.float64)
    return np.asarray(y, np.float64).reshape(-1, fw.size) @ fw


def loss_grad64(y, t, wt, fw, count_total=0):
    """-> (gy [n*K], loss, pred [n]) in float64."""
    fw = np.asarray(fw, np.float64)
    p = reduce64(y, fw)
    r = p - np.asarray(t, np.float64).reshape(-1)
    w = np.ones_like(r) if wt is None else np.asarray(wt, np.float64).reshape(-1)
    inv = 1.0 / (count_total if count_total else r.size)
    return ((2.0 * w * r * inv)[:, None] * fw[None, :]).reshape(-1), float(inv * np.sum(w * r * r)), p


def torch_loss(y, t, wt, fw):
    """The same loss in torch ops on ``y`` [n*K, 1] (any dtype / device; differentiable): mean_i(wt_i (p_i - t_i)^2)."""
    p = (y.reshape(-1, fw.numel()) * fw).sum(dim=1)
    r = p - t.reshape(-1)
    return ((r * r) if wt is None else (wt.reshape(-1) * r * r)).mean()
