// Snapshots of the simulation state on the device: rw_snapshot_create / _save / _restore / _restore_indexed / _destroy
// (include/rware_hip.h, include/rware_hip_restore.h).  Included by rware_capi.hip at file scope, after rware_kernels.h (STATUS_RESTORE_INDEX)
// and after the engine internals the host part below uses (rw_engine, fail, RW_HIP, launch, ALL_VIEWS, kKinds).  The kernel first, the host
// part below it.  Plain C++ throughout: the host-thread build of tests/emu compiles this file as it is.
#pragma once

namespace rw {

// rw_snapshot_restore_indexed: env e <- the rows a snapshot holds for env index[e], piece by piece (state_pieces; the field-major RNG
// buffer counts as six pieces of 8-byte rows).  A workgroup takes `E` consecutive DESTINATION envs: their indices are read once, into
// LDS — an index outside -1 .. B-1 becomes -1 there and sets STATUS_RESTORE_INDEX — and then every piece is walked with `lanes`
// (a power of two, by the row's length) consecutive lanes along one row and the groups of lanes along consecutive envs: for the
// 8- and 16-byte rows one lane per env, a wavefront on 64 neighbouring rows.  Source row j and destination row e start at unrelated
// addresses (110-byte shadow rows, 12-byte records), so the access width is chosen per (piece, env): the widest of 16, 8, 4 bytes
// that the two addresses share modulo and the row holds, bytes otherwise; bytes in front of the destination's first boundary of
// that width and behind the last.  Every access lies inside row j of the source and row e of the destination: the neighbours belong to
// envs that may keep their state.  Plain loads and stores; no thread returns before the barrier.
enum : int { MAX_RESTORE_PIECES = 24 };
struct RestorePiece {
    const char *src;      // the snapshot's copy of the piece
    char *dst;            // the engine's
    int32_t row_bytes;    // bytes of one env's row ...
    int32_t stride;       // ... and from one env's row to the next
    int32_t lanes_log2;   // lanes along one row: 1 << lanes_log2 (at most 64)
    int32_t rng;          // one of the six RNG columns: left alone under RW_RESTORE_KEEP_RNG
};
struct RestoreArgs {
    RestorePiece pc[MAX_RESTORE_PIECES];
    int32_t n_pieces, B, E, flags;
};
template <typename T>
__device__ __forceinline__ void copy_as(char *d, const char *s) { *reinterpret_cast<T *>(d) = *reinterpret_cast<const T *>(s); }
template <typename Dummy = void>
__global__ void __launch_bounds__(256) rware_restore_indexed_kernel(const int32_t *__restrict__ index, int32_t *status, const RestoreArgs a) {
    extern __shared__ __align__(16) int32_t smem[];   // [E] the source slot of every env of this workgroup, -1: keeps its state
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const int e0 = (int)blockIdx.x * a.E;
    const int ne = a.B - e0 < a.E ? a.B - e0 : a.E;  // (the last workgroup may be ragged; the launch has ceil(B / E) of them: ne >= 1)
    for (int i = tid; i < ne; i += nt) {
        int j = index[e0 + i];
        if (j < -1 || j >= a.B) {
            atomicOr(status, (int)STATUS_RESTORE_INDEX);
            j = -1;
        }
        smem[i] = j;
    }
    __syncthreads();
    for (int p = 0; p < a.n_pieces; ++p) {
        const RestorePiece pc = a.pc[p];
        if (pc.rng && (a.flags & 1)) continue;        // RW_RESTORE_KEEP_RNG (uniform)
        const int n = pc.row_bytes, sub = tid & ((1 << pc.lanes_log2) - 1), lanes = 1 << pc.lanes_log2;
        for (int slot = tid >> pc.lanes_log2; slot < ne; slot += nt >> pc.lanes_log2) {
            const int j = smem[slot];
            if (j < 0) continue;
            const char *const s = pc.src + (size_t)j * (size_t)pc.stride;
            char *const d = pc.dst + (size_t)(e0 + slot) * (size_t)pc.stride;
            const unsigned rel = (unsigned)(reinterpret_cast<uintptr_t>(s) ^ reinterpret_cast<uintptr_t>(d));
            const int w = !(rel & 15u) && n >= 16 ? 16 : !(rel & 7u) && n >= 8 ? 8 : !(rel & 3u) && n >= 4 ? 4 : 1;
            int head = (int)((0u - (unsigned)reinterpret_cast<uintptr_t>(d)) & (unsigned)(w - 1));  // bytes in front of d's first w-byte boundary
            if (head > n) head = n;
            const int body = (n - head) / w, tail0 = head + body * w;   // `body` w-byte pieces, then n - tail0 bytes
            const int items = head + body + (n - tail0);
            for (int i = sub; i < items; i += lanes) {
                if (i < head) {
                    d[i] = s[i];
                } else if (i < head + body) {
                    const int o = head + (i - head) * w;
                    if (w == 16) copy_as<int4>(d + o, s + o);
                    else if (w == 8) copy_as<uint64_t>(d + o, s + o);
                    else if (w == 4) copy_as<uint32_t>(d + o, s + o);
                    else d[o] = s[o];
                } else {
                    const int o = tail0 + (i - head - body);
                    d[o] = s[o];
                }
            }
        }
    }
}

}  // namespace rw

// ---- host part ----------------------------------------------------------------------------------------------------------------------

struct rw_snapshot {
    void *mem = nullptr;
    size_t bytes = 0;
};

namespace {
// the state that reset()/step() evolve, in a fixed order: where each piece lives in the engine, its size, and where it starts inside a
// snapshot (every piece on a 256-byte boundary there); `snapshot_bytes`: what a snapshot of all of them takes
struct StatePiece { void *ptr; size_t bytes, off; };
std::vector<StatePiece> state_pieces(rw_engine *eng, size_t *snapshot_bytes = nullptr) {
    // (the STATE rows of kKinds, by kind — empty without their flag; RW_BUF_OBS / RW_BUF_OBS_PACKED are outputs, not state: a restore
    //  recomputes them, OP_OBS, in the engine's format)
    std::vector<StatePiece> v;
    size_t off = 0;
    auto add = [&](void *ptr, size_t bytes) { v.push_back({ptr, bytes, off}); off += (bytes + 255) & ~(size_t)255; };
    add(eng->d_rec, (size_t)eng->prm.B * eng->prm.N * sizeof(uint32_t));  // the agents: their packed records
    add(eng->d_cnt, (size_t)eng->prm.B * 2 * sizeof(int32_t));            // steps, inactive, pending resets: the counter records
    for (const Kind &k : kKinds)
        if (k.role == STATE) add(eng->buf[k.kind].ptr, eng->buf[k.kind].bytes);
    add(eng->d_shadow, (size_t)eng->prm.B * eng->prm.HW * (eng->wide ? 2 : 1));
    if (snapshot_bytes) *snapshot_bytes = off;
    return v;
}
}  // namespace

extern "C" {

int rw_snapshot_create(rw_engine *eng, rw_snapshot **out) {
    if (!eng || !out) return RW_ERR_INVALID_ARG;
    RW_HIP(eng, hipSetDevice(eng->cfg.device_id));
    rw_snapshot *s = new (std::nothrow) rw_snapshot();
    if (!s) return fail(eng, RW_ERR_HIP, "out of host memory");
    state_pieces(eng, &s->bytes);
    if (hipMalloc(&s->mem, s->bytes) != hipSuccess) {
        delete s;
        return fail(eng, RW_ERR_HIP, "hipMalloc of a %zu-byte snapshot failed", s->bytes);
    }
    *out = s;
    return RW_OK;
}

int rw_snapshot_save(rw_engine *eng, rw_snapshot *snap) {
    if (!eng || !snap || !snap->mem) return RW_ERR_INVALID_ARG;
    RW_HIP(eng, hipSetDevice(eng->cfg.device_id));
    for (auto &pc : state_pieces(eng))
        if (pc.bytes) RW_HIP(eng, hipMemcpyAsync((char *)snap->mem + pc.off, pc.ptr, pc.bytes, hipMemcpyDeviceToDevice, eng->stream));
    return RW_OK;
}

int rw_snapshot_restore(rw_engine *eng, const rw_snapshot *snap) {
    if (!eng || !snap || !snap->mem) return RW_ERR_INVALID_ARG;
    RW_HIP(eng, hipSetDevice(eng->cfg.device_id));
    for (auto &pc : state_pieces(eng))
        if (pc.bytes) RW_HIP(eng, hipMemcpyAsync(pc.ptr, (const char *)snap->mem + pc.off, pc.bytes, hipMemcpyDeviceToDevice, eng->stream));
    eng->stale = ALL_VIEWS;  // (the views are not part of a snapshot: they are derived from what is)
    return launch(eng, eng->la, rw::OP_OBS);
}

int rw_snapshot_restore_indexed(rw_engine *eng, const rw_snapshot *snap, const int32_t *src_index_dev, int32_t flags) {
    // One launch of rware_restore_indexed_kernel and the observation launch of rw_snapshot_restore, both on the engine's stream, and
    // nothing else: the piece table and the flags travel in the kernel's arguments and the host never reads the index array, so the
    // call is legal inside a stream capture and is replayed with the graph.
    if (!eng) return RW_ERR_INVALID_ARG;
    if (!snap || !snap->mem || !src_index_dev)
        return fail(eng, RW_ERR_INVALID_ARG, "rw_snapshot_restore_indexed: NULL %s", !src_index_dev ? "src_index_dev" : "snapshot");
    if (reinterpret_cast<uintptr_t>(src_index_dev) & 3u)
        return fail(eng, RW_ERR_INVALID_ARG, "rw_snapshot_restore_indexed: src_index_dev has to be 4-byte aligned");
    if (flags & ~(int32_t)RW_RESTORE_KEEP_RNG)
        return fail(eng, RW_ERR_INVALID_ARG, "rw_snapshot_restore_indexed: unknown flag bits 0x%x", (unsigned)(flags & ~(int32_t)RW_RESTORE_KEEP_RNG));
    RW_HIP(eng, hipSetDevice(eng->cfg.device_id));
    const size_t B = (size_t)eng->prm.B;
    rw::RestoreArgs a{};
    size_t env_bytes = 0;
    auto add = [&](const char *src, void *dst, size_t row, bool rng) {
        rw::RestorePiece &pc = a.pc[a.n_pieces++];
        pc.src = src;
        pc.dst = (char *)dst;
        pc.row_bytes = pc.stride = (int32_t)row;
        while (pc.lanes_log2 < 6 && ((size_t)16 << pc.lanes_log2) < row) ++pc.lanes_log2;  // a lane per 16 bytes of the row, at most a wavefront
        pc.rng = rng ? 1 : 0;
        env_bytes += row;
    };
    for (auto &pc : state_pieces(eng)) {
        if (!pc.bytes) continue;
        const char *src = (const char *)snap->mem + pc.off;
        const bool rng = pc.ptr == eng->buf[RW_BUF_RNG].ptr;   // field-major uint64 [6][B]: six columns of 8-byte rows
        const int cols = rng ? 6 : 1;
        const size_t row = pc.bytes / B / (size_t)cols;
        if (a.n_pieces + cols > rw::MAX_RESTORE_PIECES || row * B * (size_t)cols != pc.bytes || row > 0x7fffffffu)
            return fail(eng, RW_ERR_UNSUPPORTED, "rw_snapshot_restore_indexed: a state piece of %zu bytes does not fit the piece table", pc.bytes);
        for (int c = 0; c < cols; ++c) add(src + (size_t)c * B * row, (char *)pc.ptr + (size_t)c * B * row, row, rng);
    }
    a.B = (int32_t)B;
    a.E = 64;      // a wavefront of neighbouring envs for the one-lane-per-env pieces
    a.flags = flags;
    const unsigned n_wg = (unsigned)((B + (size_t)a.E - 1) / (size_t)a.E);
    // (a workgroup that has little to copy is one wavefront)
    const unsigned threads = std::min<size_t>(B, (size_t)a.E) * env_bytes >= 16384 ? 256u : 64u;
    hipLaunchKernelGGL((rw::rware_restore_indexed_kernel<>), dim3(n_wg), dim3(threads), sizeof(int32_t) * (size_t)a.E, eng->stream, src_index_dev,
                       eng->d_status, a);
    RW_HIP(eng, hipGetLastError());
    eng->stale = ALL_VIEWS;
    return launch(eng, eng->la, rw::OP_OBS);
}

int rw_snapshot_destroy(rw_engine *eng, rw_snapshot *snap) {
    if (!eng) return RW_ERR_INVALID_ARG;
    if (!snap) return RW_OK;
    RW_HIP(eng, hipSetDevice(eng->cfg.device_id));
    RW_HIP(eng, hipStreamSynchronize(eng->stream));
    if (snap->mem) (void)hipFree(snap->mem);
    delete snap;
    return RW_OK;
}

}  // extern "C"
