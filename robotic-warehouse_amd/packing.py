"""Bit-packed FLATTENED observations (`obs_format="packed"`, RW_OBS_PACKED of include/rware_hip.h).

Every element of a FLATTENED observation except the two coordinates is 0.0 or 1.0 (rware/warehouse.py:643-673), so the engine can
write a row of `PW = 1 + ceil(L / 32)` uint32 words per agent instead of L floats:

    word 0                        x | y << 16   (cell indices, whatever `normalised_coordinates` says)
    word 1 + k // 32, bit k % 32  obs[k] != 0   for 2 <= k < L   (bits 0, 1 of word 1 and the bits from L on are 0)

`unpack_obs` is the inverse a learner calls on a minibatch (numpy in -> numpy out; torch in -> torch out on the same device, plain
shift / and / cast ops, any leading dimensions) and reproduces the float32 observation bit for bit; `pack_obs` (numpy) is what the
tests pack the reference's observations with.
"""
from __future__ import annotations

import numpy as np

from .layout import obs_length


def packed_words(sensor_range: int, msg_bits: int = 0) -> int:
    """PW: uint32 words of one agent's packed row."""
    return 1 + (obs_length(sensor_range, msg_bits) + 31) // 32


def _dims(grid_size):
    h, w = int(grid_size[0]), int(grid_size[1])  # grid_size is (H, W) as in the reference (rware/warehouse.py:297-300)
    return h, w


def pack_obs(obs, grid_size, sensor_range, msg_bits=0, normalised_coordinates=False):
    """float32 (..., L) FLATTENED observations -> uint32 (..., PW).  Raises if an element past the coordinates is neither 0 nor 1."""
    obs = np.asarray(obs, dtype=np.float32)
    L = obs_length(sensor_range, msg_bits)
    if obs.shape[-1] != L:
        raise ValueError(f"expected observations of length {L}, got {obs.shape[-1]}")
    H, W = _dims(grid_size)
    body = obs[..., 2:]
    if not np.all((body == 0.0) | (body == 1.0)):
        raise ValueError("a FLATTENED observation holds only 0 / 1 past its two coordinates")
    xy = obs[..., :2].astype(np.float64)
    if normalised_coordinates:  # obs = float32(v / (dim - 1)): the nearest integer gives v back (dim <= 65536)
        xy = xy * np.array([W - 1, H - 1], np.float64)
    xy = np.rint(xy).astype(np.int64)
    if xy.size and (xy.min() < 0 or xy[..., 0].max() >= max(W, 1) or xy[..., 1].max() >= max(H, 1)):
        raise ValueError("coordinates outside the grid")
    ow = (L + 31) // 32
    bits = np.zeros(obs.shape[:-1] + (32 * ow,), np.uint32)
    bits[..., 2:L] = body != 0.0
    words = (bits.reshape(obs.shape[:-1] + (ow, 32)) << np.arange(32, dtype=np.uint32)).sum(-1, dtype=np.uint64).astype(np.uint32)
    out = np.empty(obs.shape[:-1] + (1 + ow,), np.uint32)
    out[..., 0] = (xy[..., 0] | (xy[..., 1] << 16)).astype(np.uint32)
    out[..., 1:] = words
    return out


def unpack_obs(packed, grid_size, sensor_range, msg_bits=0, normalised_coordinates=False):
    """uint32 (..., PW) packed rows -> float32 (..., L), bit for bit the engine's float32 observation.  numpy in -> numpy out; a torch
    tensor (uint32 bit patterns held as int32 — what the zero-copy views are — or any integer dtype) -> a torch tensor on its device."""
    L = obs_length(sensor_range, msg_bits)
    ow = (L + 31) // 32
    H, W = _dims(grid_size)
    if isinstance(packed, np.ndarray) or not hasattr(packed, "device"):
        p = np.asarray(packed)
        if p.shape[-1] != 1 + ow:
            raise ValueError(f"expected packed rows of {1 + ow} words, got {p.shape[-1]}")
        p = p.astype(np.uint32, copy=False)
        out = np.empty(p.shape[:-1] + (L,), np.float32)
        bits = (p[..., 1:, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
        out[...] = bits.reshape(p.shape[:-1] + (32 * ow,))[..., :L]
        x, y = p[..., 0] & np.uint32(0xFFFF), p[..., 0] >> np.uint32(16)
        if normalised_coordinates:  # float32(float64(v) / float64(dim - 1)): coordf of the step kernel (rware/warehouse.py:636-638)
            with np.errstate(divide="ignore", invalid="ignore"):
                out[..., 0] = (x.astype(np.float64) / np.float64(W - 1)).astype(np.float32)
                out[..., 1] = (y.astype(np.float64) / np.float64(H - 1)).astype(np.float32)
        else:
            out[..., 0] = x
            out[..., 1] = y
        return out
    import torch

    p = packed
    if p.shape[-1] != 1 + ow:
        raise ValueError(f"expected packed rows of {1 + ow} words, got {p.shape[-1]}")
    if p.dtype != torch.int32:  # (uint32 has no shift ops in torch: same bits as int32; wider integers keep the low 32)
        p = p.view(torch.int32) if p.dtype == getattr(torch, "uint32", None) else p.to(torch.int64).to(torch.int32)
    sh = torch.arange(32, dtype=torch.int32, device=p.device)
    bits = (p[..., 1:, None] >> sh) & 1  # (arithmetic shift: the mask drops the copies of the sign bit)
    out = bits.reshape(p.shape[:-1] + (32 * ow,))[..., :L].to(torch.float32)
    x, y = p[..., 0] & 0xFFFF, (p[..., 0] >> 16) & 0xFFFF
    if normalised_coordinates:
        out[..., 0] = (x.to(torch.float64) / float(W - 1)).to(torch.float32)
        out[..., 1] = (y.to(torch.float64) / float(H - 1)).to(torch.float32)
    else:
        out[..., 0] = x.to(torch.float32)
        out[..., 1] = y.to(torch.float32)
    return out
