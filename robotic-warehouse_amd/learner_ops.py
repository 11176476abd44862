"""What a learner calls between steps, as a mixin of `WarehouseVecEnv`: snapshots (restore / clone by index), packed minibatches, the
critic's global state, advantages and returns.  Every device operation only ENQUEUES on the env's stream.  Two dicts on the env: `_op_cache` (what an operation
allocated, per key) and `_op_live` (the arguments of its last launch, alive until its next call)."""
from __future__ import annotations

import numpy as np

from . import _capi
from .advantages import gae_shapes
from .enums import ImageLayer, ObservationType, enum_value
from .layout import obs_length
from .packing import packed_words, unpack_obs as _unpack_obs


def global_image_from_state(state, goals, image_layers, pad_to_shape=None):
    """`Warehouse.get_global_image` (rware/warehouse.py:966-1040) from a batched get_state() dict: (B, C, H, W) float32.
    Same quirks: GOALS written as the reference does (its loop variables are swapped twice: the right cells, :1013-1015);
    AGENT_DIRECTION / AGENT_LOAD indexed `[ag.x, ag.y]` on an (H, W) array (:1003-1011) — the mirrored cell, IndexError when
    x >= H or y >= W; REQUESTS from the positions of the queued shelves; padding split as in :1023-1039."""
    grid = np.asarray(state["grid"])
    B, _, H, W = grid.shape
    ax, ay = np.asarray(state["agent_x"]), np.asarray(state["agent_y"])
    rows = np.arange(B)[:, None]
    layers = []
    for lt in image_layers:
        lt = ImageLayer(enum_value(lt))
        layer = np.zeros((B, H, W), np.float32)
        if lt == ImageLayer.SHELVES:
            layer[grid[:, 1] > 0] = 1.0
        elif lt == ImageLayer.REQUESTS:
            q = np.asarray(state["queue"])
            for k in range(q.shape[1]):
                layer[np.asarray(grid[:, 1] == q[:, k, None, None]) & (q[:, k, None, None] > 0)] = 1.0
        elif lt == ImageLayer.AGENTS:
            layer[grid[:, 0] > 0] = 1.0
        elif lt in (ImageLayer.AGENT_DIRECTION, ImageLayer.AGENT_LOAD):
            carry = np.asarray(state["agent_carry"])
            use = np.ones_like(ax, bool) if lt == ImageLayer.AGENT_DIRECTION else carry > 0
            if ((ax >= H) | (ay >= W))[use].any():
                raise IndexError("index out of bounds: AGENT_DIRECTION / AGENT_LOAD are written at [ag.x, ag.y] (rware/warehouse.py:1006,1011)")
            val = (np.asarray(state["agent_dir"]) + 1).astype(np.float32) if lt == ImageLayer.AGENT_DIRECTION else np.ones_like(ax, np.float32)
            for i in range(ax.shape[1]):  # agent order: a later agent overwrites an earlier one on the same (mirrored) cell
                m = use[:, i]
                layer[rows[m, 0], ax[m, i], ay[m, i]] = val[m, i]
        elif lt == ImageLayer.GOALS:
            for gx, gy in goals:
                layer[:, gy, gx] = 1.0
        elif lt == ImageLayer.ACCESSIBLE:
            layer[:] = 1.0
            layer[rows, ay, ax] = 0.0
        layers.append(layer)
    img = np.stack(layers, axis=1)
    if pad_to_shape is not None:
        pad = [p - g for p, g in zip(pad_to_shape, img.shape[1:])]
        assert all(d >= 0 for d in pad)
        img = np.pad(img, ((0, 0),) + tuple((d // 2, d // 2 if d % 2 == 0 else d // 2 + 1) for d in pad), mode="constant", constant_values=0)
    return img


def _is_tensor_arg(x):
    """A torch tensor, or a non-empty list / tuple of them (one per shard) — told by duck typing: torch is imported only by output="torch" envs."""
    if isinstance(x, (list, tuple)):
        return bool(x) and all(hasattr(v, "is_cuda") and hasattr(v, "data_ptr") for v in x)
    return hasattr(x, "is_cuda") and hasattr(x, "data_ptr")


def _resolve_dtype(t, dtype, codes):
    """A `dtype` argument — a name in `codes` (name -> C element code) or the torch dtype of that name — -> (torch dtype, code)."""
    by_name = {n: getattr(t, n) for n in codes}
    tdt = by_name.get(dtype, dtype) if isinstance(dtype, str) else dtype
    if tdt not in by_name.values():
        listing = ", ".join(f'"{n}"' for n in list(codes)[:-1]) + f' or "{list(codes)[-1]}"'
        raise ValueError(f"dtype must be {listing} (or the torch dtype), got {dtype!r}")
    return tdt, codes[str(tdt).split(".")[-1]]


def _check_index(t, index, src, src_name, over):
    """A minibatch index against the tensor `src` (the argument `src_name`) it selects from -> its length."""
    if not hasattr(index, "is_cuda") or index.dtype not in (t.int32, t.int64) or index.dim() != 1 or not index.is_contiguous():
        raise ValueError(f"`index` must be a contiguous 1-D int32 or int64 tensor over {over}")
    if index.device != src.device:
        raise ValueError(f"`index` lives on {index.device}, `{src_name}` on {src.device}")
    return int(index.shape[0])


def _check_out(o, shape, tdt, device, what, where, aligned=False):
    """A caller's `out` (or one of the cached ones): a contiguous tensor of this shape and dtype on this device, 16-byte aligned if asked."""
    if not (hasattr(o, "is_cuda") and tuple(o.shape) == tuple(shape) and o.dtype == tdt and o.device == device and o.is_contiguous()
            and not (aligned and o.data_ptr() % 16)):
        raise ValueError(f"`out` must be a {what} of shape {tuple(shape)} on {where}")


class LearnerOps:
    # ------------------------------------------------------------------------------- helpers, each written once
    def _cached(self, key, make):
        """What an operation allocated on its first call per `key` = (op, device, shape, dtype, ...), overwritten by later calls."""
        got = self._op_cache.get(key)
        if got is None:
            got = self._op_cache[key] = make()
        return got

    def _release_learner_ops(self):
        """close(): clone_envs' snapshot is freed; what the operations allocated and kept alive is let go."""
        token = self._op_cache.pop("clone_token", None)
        if token is not None and self.engines:
            self.free_snapshot(token)
        self._op_cache, self._op_live = {}, {}

    def _image_shape(self, who, image_layers, pad_to_shape):
        """-> (layer values, (C', H', W'), pad_to_shape as ints or None); ValueError and AssertionError as rware/warehouse.py:1018, :1028."""
        layers = tuple(ImageLayer(enum_value(l)).value for l in image_layers)
        if not 1 <= len(layers) <= 8:
            raise ValueError(f"{who} takes 1 to 8 image layers")
        shape = (len(layers),) + tuple(self.grid_size)
        if pad_to_shape is not None:
            pad_to_shape = tuple(int(v) for v in pad_to_shape)
            assert len(pad_to_shape) == 3 and all(p >= s for p, s in zip(pad_to_shape, shape))
            shape = pad_to_shape
        return layers, shape, pad_to_shape

    def _minibatch_out(self, op, src, name, hint, out, shape, tdt):
        """-> (the engine on the device of the CUDA tensor `src`, argument `name` of method `op`; the caller's `out`, checked, or the tensor
        allocated on the first call per (op, device, shape, dtype))."""
        if out is not None:
            _check_out(out, shape, tdt, src.device, f"contiguous {tdt} tensor", src.device)
        if not src.is_cuda:
            raise ValueError(f"`{name}` is a host tensor: {op} works on the device{hint}")
        if self.output != "torch":
            raise ValueError(f'{op} needs output="torch": only such an env enqueues on the stream the tensors are ordered on')
        if src.device.index not in self.devices:
            raise ValueError(f"no engine of this env runs on {src.device}")
        if out is None:
            out = self._cached((op, src.device.index, shape, tdt), lambda: self._torch.empty(shape, dtype=tdt, device=src.device))
        return self.engines[self.devices.index(src.device.index)], out

    def _shard_outputs(self, op, key, out, shape_of, dtype, what, launch, aligned=False):
        """launch(engine, device pointer) once per shard.  output="torch": into the caller's `out` (a tensor, or a list with one per device)
        or the tensors allocated on the first call per `key`, each checked -> the tensor, a tuple of them when sharded.  numpy: _via_scratch."""
        if self.output != "torch":
            return self._via_scratch(op, out, shape_of, dtype, launch)
        t = self._torch
        tdt = getattr(t, np.dtype(dtype).name)
        outs = list(out) if isinstance(out, (list, tuple)) else [out]
        if out is None:
            outs = self._cached((op,) + key, lambda: [t.empty(shape_of(eng), dtype=tdt, device=f"cuda:{dev}") for eng, dev in zip(self.engines, self.devices)])
        if len(outs) != len(self.engines):
            raise ValueError(f"`out` must hold one tensor per device ({len(self.engines)})")
        for eng, dev, o in zip(self.engines, self.devices, outs):
            _check_out(o, shape_of(eng), tdt, t.device("cuda", dev), what.format(tdt), f"device {dev}", aligned)
        for eng, o in zip(self.engines, outs):
            launch(eng, o.data_ptr())
        self._op_live[op] = outs  # (a caller's `out` stays alive until the next call: the launch is only enqueued)
        return outs[0] if len(outs) == 1 else tuple(outs)

    def _via_scratch(self, name, out, shape_of, dtype, launch):
        """numpy output: launch(engine, pointer) into every engine's scratch array, sync() on EVERY shard — the first error is raised
        afterwards, so that no shard keeps a raised flag for a later call —, and a host array gathered over the shards."""
        if out is not None:
            raise ValueError('`out` is a device tensor: it exists with output="torch" only')
        parts = [np.empty(shape_of(eng), dtype) for eng in self.engines]
        for eng, part in zip(self.engines, parts):
            launch(eng, eng.scratch(name, part.nbytes).value)
        err = None
        for eng in self.engines:
            try:
                eng.sync()
            except (IndexError, ValueError) as e:
                err = err or e
        if err is not None:
            raise err
        for eng, part in zip(self.engines, parts):
            eng.read_scratch(name, part)
        return parts[0] if len(parts) == 1 else np.concatenate(parts, axis=0)

    # ------------------------------------------------------------------------------- snapshots
    def snapshot(self):
        """Checkpoint the batched state on the device (grid, agents, queue, counters, RNG streams).
        Returns an opaque token for restore(); free it with free_snapshot()."""
        return [eng.snapshot() for eng in self.engines]

    def restore(self, token, index=None, keep_rng=False):
        """Roll every env back to a snapshot(); the engine then continues bit-identically.

        `index` (B,): env e takes the state the snapshot holds for env index[e]; -1 keeps env e as it is; repeats are allowed (all
        zeros broadcasts slot 0 to every env).  The copy is a kernel on the env's stream (rw_snapshot_restore_indexed) followed by the
        observation launch: the call only enqueues.  Two forms:
          - a CUDA int32 tensor (B,) on the env's device (output="torch"): zero-copy, nothing waits — legal behind a policy and inside
            capture_loop; int64 is converted with .to(torch.int32); a multi-device env takes a list of one SHARD-LOCAL tensor per
            device.  A value outside -1 .. B-1 leaves that env untouched and raises at the next sync();
          - a host integer array of GLOBAL env indices (any output mode): checked here (ValueError for a value outside -1 .. B-1 and
            for a source on another shard than its destination), made shard-local and uploaded into a buffer each engine keeps.
        `keep_rng`: every env's RNG stream stays as it is, so clones of one state draw different request replacements; without it
        clones are identical and stay so under identical actions.  rewards / terminated / truncated are outputs of a step and are
        left as they are.  Returns the observations, as restore(token) does."""
        if index is None:
            if keep_rng:
                raise ValueError("keep_rng applies to an indexed restore: pass index=")
            for eng, h in zip(self.engines, token):
                eng.restore(h)
            return self._observations()
        ptrs, keep = self._restore_index(index)
        for eng, h, p in zip(self.engines, token, ptrs):
            eng.restore_indexed(h, p, keep_rng)
        self._op_live["restore"] = keep  # alive until the next indexed restore replaces them (stream-ordered allocator: see step_async)
        return self._observations()

    def _restore_index(self, index):
        """restore()'s index, checked -> (one device pointer per shard, what has to stay alive).  Nothing here waits for the device
        when the index is a tensor."""
        t, n = self._torch, len(self.engines)
        tensors = _is_tensor_arg(index)
        if tensors:
            if t is None:
                raise ValueError('a tensor index needs output="torch": only such an env enqueues on the stream the tensor is ordered on')
            parts = list(index) if isinstance(index, (list, tuple)) else [index]
            if len(parts) != n:
                raise ValueError(f"expected {n} per-device index tensors (shard-local indices), got {len(parts)}")
            out = []
            for d, (v, (lo, hi)) in enumerate(zip(parts, self._bounds)):
                if not v.is_cuda or v.device.index != self.devices[d]:
                    raise ValueError(f"the index tensor of shard {d} must live on cuda:{self.devices[d]}")
                if tuple(v.shape) != (hi - lo,):
                    raise ValueError(f"the index tensor of shard {d} must have shape ({hi - lo},), got {tuple(v.shape)}")
                if v.dtype not in (t.int32, t.int64):
                    raise ValueError(f"the index tensor must be int32 or int64, got {v.dtype}")
                out.append(v.to(t.int32).contiguous())
            return [v.data_ptr() for v in out], out
        h = np.asarray(index)
        if h.dtype.kind not in "iu" or h.shape != (self.num_envs,):
            raise ValueError(f"index must be an integer array of shape ({self.num_envs},), got {h.dtype} {h.shape}")
        h = h.astype(np.int64)
        if ((h < -1) | (h >= self.num_envs)).any():
            raise ValueError(f"index values must lie in -1 .. {self.num_envs - 1}")
        local = []
        for lo, hi in self._bounds:
            part = h[lo:hi]
            if ((part >= 0) & ((part < lo) | (part >= hi))).any():
                raise ValueError("an env can only take a state saved on its own device: a source index on another shard (a cross-device "
                                 "copy is not supported)")
            local.append(np.where(part >= 0, part - lo, -1).astype(np.int32))
        return [eng.upload_index(part) for eng, part in zip(self.engines, local)], None

    def _alloc_clone_token(self):
        """clone_envs' snapshot: allocated on first use, freed in close()."""
        return self._cached("clone_token", lambda: [eng.create_snapshot() for eng in self.engines])

    def clone_envs(self, index, keep_rng=False):
        """Env e becomes a copy of env index[e] AS IT IS NOW (-1: stays itself): a snapshot into a token the env keeps (allocated on
        first use, freed in close()), then restore(token, index, keep_rng).  Both halves only enqueue, so with a device tensor it
        can be called behind a policy and inside capture_loop.  `index` and `keep_rng`: as for restore().  Returns the observations."""
        ptrs, keep = self._restore_index(index)   # (checked before anything is enqueued)
        token = self._alloc_clone_token()
        for eng, h in zip(self.engines, token):
            eng.snapshot(into=h)
        for eng, h, p in zip(self.engines, token, ptrs):
            eng.restore_indexed(h, p, keep_rng)
        self._op_live["restore"] = keep
        return self._observations()

    def free_snapshot(self, token):
        for eng, h in zip(self.engines, token):
            eng.free_snapshot(h)

    # ------------------------------------------------------------------------------- packed minibatches
    def unpack_obs(self, packed):
        """Packed rows (..., PW) -> float32 (..., L) with this env's parameters: bit for bit what obs_format="float32" returns.  numpy in
        -> numpy out; a torch tensor -> a torch tensor on the same device (plain shift / and / cast ops: call it on a minibatch)."""
        return _unpack_obs(packed, self.grid_size, self.sensor_range, self.msg_bits, self.normalised_coordinates)

    def unpack_obs_device(self, packed, index=None, dtype="float32", out=None):
        """unpack_obs(packed[index]).to(dtype) in ONE kernel on the env's stream (rw_unpack_obs_gather), without the gathered copy and the
        intermediates of the tensor-op path: the learner's half of obs_format="packed".  output="torch" only.
        `packed`: a contiguous CUDA int32 (or uint32) tensor (G0, ..., PW) — a rollout tape reshaped to (T*B, N, PW), the live
        "obs_packed" (B, N, PW), or plain rows (n, PW); `index`: a 1-D CUDA int32 or int64 tensor over the FIRST dimension (repeats
        allowed; None: the whole array); `dtype`: "float32" | "float16" | "bfloat16" or the torch dtype — float32 is bit for bit what
        obs_format="float32" returns, the 16-bit types are that value rounded to nearest even (0 and 1 are exact: only the two
        coordinates round).  Returns a tensor (n, ..., L): `out` if given (contiguous, of that shape and dtype, on `packed`'s device), else
        one allocated on the first call per (shape, dtype) and overwritten by later ones.  With several devices the tensor's device picks
        the engine.  The call only enqueues — on the stream step() uses, so it is ordered with the learner like every other call and a
        policy inside capture_loop may make it (a replay reads the index tensor's contents at replay time).  An index outside
        0 .. G0-1 gives rows of zeros and raises at the next sync().  ValueError for a host tensor, a wrong last dimension, a
        non-contiguous input, an `out` of the wrong shape, dtype or device."""
        if self.observation_type in (ObservationType.IMAGE, ObservationType.IMAGE_DICT):
            raise ValueError("packed rows exist for FLATTENED observations only")
        if not (hasattr(packed, "is_cuda") and hasattr(packed, "data_ptr")):
            raise ValueError("unpack_obs_device takes torch tensors (numpy rows: unpack_obs)")
        import torch as t

        tdt, elem = _resolve_dtype(t, dtype, _capi.UNPACK_ELEMS)
        L, pw = obs_length(self.sensor_range, self.msg_bits), packed_words(self.sensor_range, self.msg_bits)
        if packed.dtype not in (t.int32, getattr(t, "uint32", t.int32)):
            raise ValueError(f"packed rows are int32 (or uint32) words, got {packed.dtype}")
        if packed.dim() < 2 or packed.shape[-1] != pw:
            raise ValueError(f"expected packed rows (G0, ..., {pw}), got {tuple(packed.shape)}")
        if not packed.is_contiguous():
            raise ValueError("`packed` must be contiguous (reshape a tape, do not slice or transpose it)")
        g0, rows = int(packed.shape[0]), int(np.prod(packed.shape[1:-1], dtype=np.int64))
        n = g0 if index is None else _check_index(t, index, packed, "packed", "the first dimension of `packed`")
        shape = (n,) + tuple(packed.shape[1:-1]) + (L,)
        eng, out = self._minibatch_out("unpack_obs_device", packed, "packed", " (host rows: unpack_obs)", out, shape, tdt)
        if out.numel():  # (an empty index or an empty middle dimension: nothing to write)
            eng.unpack_gather(packed.data_ptr(), g0, rows, None if index is None else index.data_ptr(), n, elem,
                              index is not None and index.dtype == t.int64, out.data_ptr())
        self._op_live["unpack_obs_device"] = (packed, index, out)  # (alive until the next call: the launch is only enqueued)
        return out

    # ------------------------------------------------------------------------------- the critic's global state
    def get_global_image(self, image_layers=(ImageLayer.SHELVES, ImageLayer.GOALS), recompute=False, pad_to_shape=None):
        """Warehouse.get_global_image (:966-1040) for every env: float32 (B, C, H, W) (or (B,) + pad_to_shape), layer by layer
        as the reference builds them — including its cache (`recompute=False` returns the last image, whatever layers it was
        built with) and the transposed AGENT_DIRECTION / AGENT_LOAD layers (IndexError where the reference raises it).
        Host-side, from get_state(): a global-state input for centralised critics, not part of the per-step path."""
        if not recompute and getattr(self, "global_image", None) is not None:
            return self.global_image
        st = self.get_state()
        self.global_image = global_image_from_state(st, self.goals, image_layers, pad_to_shape)
        return self.global_image

    def global_image_device(self, image_layers=(ImageLayer.SHELVES, ImageLayer.GOALS), pad_to_shape=None, dtype="float32", out=None):
        """get_global_image built ON THE DEVICE (rw_global_image): the same image, layer for layer — (B, C, H, W), or (B,) + pad_to_shape —
        as float32 or uint8 (`dtype`; every element is an integer in 0 .. 4), from the state the current observation describes.  One
        kernel on the env's stream, which reads what the step kernels keep: no get_state(), no copy of the grid, no cache (every call
        recomputes; get_global_image and its cache are untouched).
        output="torch": a CUDA tensor, allocated on the first call per (layers, shape, dtype) and overwritten in place by later ones — or
        `out`, a contiguous CUDA tensor of that shape and dtype (a slice at any element offset will do).  Nothing waits and nothing
        visits the host, so a policy inside capture_loop may call it (into a preallocated `out`); the reference's IndexError for the
        AGENT_DIRECTION / AGENT_LOAD layers (an agent at x >= H or y >= W) surfaces at the next sync(), and such an agent writes nothing.
        A sharded env returns one tensor per device (`out`: one per device).
        numpy output: the same kernel into a device scratch array of the engine's, then sync() — IndexError where the reference raises
        it — and a host array gathered over the shards.
        AssertionError for a pad_to_shape smaller than the image (:1028), ValueError for an unknown layer (:1018)."""
        layers, shape, pad_to_shape = self._image_shape("global_image_device", image_layers, pad_to_shape)
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.uint8)):
            raise ValueError('dtype must be "float32" or "uint8"')
        return self._shard_outputs("global_image", (layers, shape, dt.str), out, lambda eng: (eng.B,) + shape, dt, "contiguous {} CUDA tensor",
                                   lambda eng, ptr: eng.global_image(layers, ptr, pad_to_shape, dt))

    @property
    def global_record_bytes(self) -> int:
        """RB = (H*W + 1 + 15) & ~15: the bytes of one env's global-state record (global_records_device)."""
        return self.engines[0].global_record_bytes

    def global_records_device(self, out=None):
        """The critic's global state as BYTE RECORDS (rw_global_records): uint8 (B, RB), one record per env — byte y*W + x the code of cell
        (x, y) (bit 0 shelf, 1 requested, 2 agent, 3 goal, 4 AGENT_LOAD and 5..7 AGENT_DIRECTION on the mirrored cell), byte H*W two flags
        (an agent / a carrying agent without a mirrored cell), zeros up to RB (include/rware_hip_global_state.h).  Every layer of
        get_global_image at about one byte per cell: keep a (T, B, RB) tape of these instead of images and expand only the minibatches
        the critic draws (global_image_from_records).  One kernel on the env's stream, from the state the current observation describes;
        it never raises — whether the AGENT_DIRECTION / AGENT_LOAD layers are asked for is decided when records are gathered.
        output="torch": a CUDA tensor allocated on the first call and overwritten by later ones — or `out`, a contiguous uint8 CUDA tensor
        (B, RB) whose address is 16-byte aligned (a slot of a (T, B, RB) tape is).  Enqueue only: a policy inside capture_loop may call
        it (into a preallocated `out`).  A sharded env returns one tensor per device (`out`: one per device).
        numpy output: the same kernel into a device scratch array of the engine's, then sync(), and a host array gathered over the shards."""
        rb = self.global_record_bytes
        return self._shard_outputs("global_records", (), out, lambda eng: (eng.B, rb), np.uint8, "contiguous, 16-byte aligned uint8 CUDA tensor",
                                   lambda eng, ptr: eng.global_records(ptr), aligned=True)

    def global_image_from_records(self, records, index=None, image_layers=(ImageLayer.SHELVES, ImageLayer.GOALS), pad_to_shape=None,
                                  dtype="float32", out=None):
        """global_image_device for a MINIBATCH of stored records (rw_global_image_gather): image i is the image of record index[i], layer
        for layer what get_global_image gave for the state that record was taken from.  output="torch" only.
        `records`: a contiguous CUDA uint8 tensor (..., RB) — a (T, B, RB) tape counts as T*B records; `index`: a 1-D CUDA int32 or int64
        tensor over the flattened records (repeats allowed; None: all of them, in order); `dtype`: "float32" | "uint8" | "float16" |
        "bfloat16" or the torch dtype (every value is an integer in 0 .. 4, exact in all four).  Returns a tensor (n, C', H', W'): `out`
        if given (contiguous, of that shape and dtype, on `records`' device; any element offset will do), else one allocated on the
        first call per (shape, dtype, device) and overwritten by later ones.  With several devices the tensor's device picks the engine.
        The call only enqueues, on the stream step() uses; a policy inside capture_loop may make it.  At the next sync(): an error
        (RW_ERR_INVALID_ARG, as for unpack_obs_device) for an index outside 0 .. n-1 (that image is zeros), IndexError where a gathered record's state made the reference raise for a
        requested AGENT_DIRECTION / AGENT_LOAD layer (that agent wrote nothing).
        AssertionError for a pad_to_shape smaller than the image, ValueError for an unknown layer or dtype, a host tensor, a wrong last
        dimension, a non-contiguous input, an `out` of the wrong shape, dtype or device."""
        layers, shape, pad_to_shape = self._image_shape("global_image_from_records", image_layers, pad_to_shape)
        if not (hasattr(records, "is_cuda") and hasattr(records, "data_ptr")):
            raise ValueError("global_image_from_records takes torch tensors")
        import torch as t

        tdt, elem = _resolve_dtype(t, dtype, _capi.GLOBAL_ELEMS)
        rb = self.global_record_bytes
        if records.dtype != t.uint8:
            raise ValueError(f"records are uint8, got {records.dtype}")
        if records.dim() < 1 or records.shape[-1] != rb:
            raise ValueError(f"expected records (..., {rb}), got {tuple(records.shape)}")
        if not records.is_contiguous():
            raise ValueError("`records` must be contiguous (do not slice the last dimension or transpose a tape)")
        n_records = int(np.prod(records.shape[:-1], dtype=np.int64))
        n = n_records if index is None else _check_index(t, index, records, "records", "the flattened records")
        shape = (n,) + shape
        if records.data_ptr() % 16:
            raise ValueError("`records` must start on a 16-byte boundary")
        eng, out = self._minibatch_out("global_image_from_records", records, "records", "", out, shape, tdt)
        if n:  # (an empty index: nothing to write)
            eng.global_image_gather(records.data_ptr(), n_records, None if index is None else index.data_ptr(), n, layers, out.data_ptr(),
                                    pad_to_shape, elem, index is not None and index.dtype == t.int64)
        self._op_live["global_image_from_records"] = (records, index, out)  # (alive until the next call: the launch is only enqueued)
        return out

    # ------------------------------------------------------------------------------- advantages and returns
    def gae_device(self, rewards, values, terminated, truncated=None, last_values=None, final_values=None, prev_ended=None, gamma=0.99,
                   lam=0.95, team_reward=None, next_step=None, out=None):
        """GAE(lambda) advantages and returns of a rollout's tapes in ONE kernel on the env's stream (rw_gae) instead of a backward loop of
        T times five to eight small tensor ops: -> (advantages, returns, valid).  output="torch" only; all arguments CUDA tensors on one
        device, contiguous.  The numbers are those of rware_amd.gae, bit for bit (include/rware_hip_advantages.h fixes every operation).
        `rewards`: float32 (T, B, N), the rollout's reward tape.  `values`: float32 (T+1, B, K) or (T+1, B) — V of the observation each
        step acted on, row T V of the observation after the last step, read in place — or (T, B, K) / (T, B) with `last_values` (B, K) /
        (B,); K == N a per-agent critic, K == 1 one value per env.  `terminated`, `truncated` (None: none), `prev_ended`: bool or uint8
        (reinterpreted, not cast), (T, B), (T, B) and (B,).
        `next_step` (None: this env's autoreset mode): the tape was written under NEXT_STEP autoreset — the step after an episode end is
        a reset step: advantage 0, returns == values and valid False there; a truncated end bootstraps from values[t + 1], which is
        V(final obs) in that mode; `prev_ended`, terminated | truncated of the last row of the tape BEFORE this one, says whether step
        0 is a reset step (None: no).  Otherwise (SAME_STEP, or DISABLED with a masked reset in the loop) a truncated end bootstraps
        from `final_values` — V(final_obs), the shape of values[:T], read only where truncated and not terminated — or from 0.
        `team_reward` (None: K == 1 and N > 1): every head sees the env's summed reward.
        Returns float32 advantages and returns of the shape of values[:T] and a bool (T, B) mask: `out`, a triple of such tensors
        (slices of larger buffers will do as long as they are contiguous), else tensors allocated on the first call per shape and
        overwritten by later ones.  With several devices the device of `rewards` picks the engine; B is the tape's, not the env's.
        The call only enqueues, on the stream step() uses; a policy inside capture_loop or any captured region may make it (a replay
        reads the tensors' contents at replay time).  ValueError for host tensors, wrong shapes or dtypes, non-contiguous inputs, an
        `out` of the wrong shape, dtype or device, gamma or lam outside [0, 1]."""
        if not all(hasattr(x, "is_cuda") and hasattr(x, "data_ptr") for x in (rewards, values, terminated)):
            raise ValueError("gae_device takes torch tensors (numpy tapes: rware_amd.gae)")
        import torch as t

        is_t = lambda x: hasattr(x, "is_cuda") and hasattr(x, "data_ptr")
        T, B, N, K, shape = gae_shapes(tuple(rewards.shape), tuple(values.shape), None if last_values is None else tuple(getattr(last_values, "shape", ())))
        if not (0.0 <= float(gamma) <= 1.0 and 0.0 <= float(lam) <= 1.0):
            raise ValueError(f"gamma ({gamma}) and lam ({lam}) must lie in [0, 1]")
        team = (K == 1 and N > 1) if team_reward is None else bool(team_reward)
        if K == 1 and N > 1 and not team:
            raise ValueError("one value head over several agents needs team_reward")
        ns = self.autoreset_mode == "next_step" if next_step is None else bool(next_step)
        given = {"rewards": (rewards, (T, B, N), (t.float32,)), "values": (values, tuple(values.shape), (t.float32,)),
                 "terminated": (terminated, (T, B), (t.bool, t.uint8)), "truncated": (truncated, (T, B), (t.bool, t.uint8)),
                 "last_values": (last_values, shape[1:], (t.float32,)), "final_values": (final_values, shape, (t.float32,)),
                 "prev_ended": (prev_ended, (B,), (t.bool, t.uint8))}
        for name, (x, want, dtypes) in given.items():
            if x is None:
                continue
            if not is_t(x) or tuple(x.shape) != tuple(want) or x.dtype not in dtypes:
                raise ValueError(f"`{name}` must be a {' or '.join(str(d) for d in dtypes)} tensor of shape {tuple(want)}, got "
                                 f"{getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}")
            if not x.is_contiguous():
                raise ValueError(f"`{name}` must be contiguous")
            if x.device != rewards.device:
                raise ValueError(f"`{name}` lives on {x.device}, `rewards` on {rewards.device}")
        if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 3):
            raise ValueError("`out` must be a triple (advantages, returns, valid)")
        o_adv, o_ret, o_valid = out if out is not None else (None, None, None)
        dev = rewards.device
        eng, adv = self._minibatch_out("gae_device", rewards, "rewards", " (host tapes: rware_amd.gae)", o_adv, shape, t.float32)
        if out is None:
            ret = self._cached(("gae_device", "returns", dev.index, shape), lambda: t.empty(shape, dtype=t.float32, device=dev))
            valid = self._cached(("gae_device", "valid", dev.index, (T, B)), lambda: t.empty((T, B), dtype=t.bool, device=dev))
        else:
            ret, valid = o_ret, o_valid
            _check_out(ret, shape, t.float32, dev, "contiguous float32 tensor (returns)", dev)
            _check_out(valid, (T, B), t.bool, dev, "contiguous bool tensor (valid)", dev)
        ptr = lambda x: 0 if x is None else x.data_ptr()
        last_ptr = values.data_ptr() + T * B * K * 4 if last_values is None else last_values.data_ptr()   # (row T, in place)
        eng.gae(rewards.data_ptr(), values.data_ptr(), last_ptr, terminated.data_ptr(), adv.data_ptr(), T, B, N, K,
                truncated_ptr=ptr(truncated), final_values_ptr=ptr(final_values), prev_ended_ptr=ptr(prev_ended), returns_ptr=ret.data_ptr(),
                valid_ptr=valid.data_ptr(), gamma=gamma, lam=lam, next_step=ns, team_reward=team)
        # (alive until the next call: the launch is only enqueued)
        self._op_live["gae_device"] = (rewards, values, terminated, truncated, last_values, final_values, prev_ended, adv, ret, valid)
        return adv, ret, valid
