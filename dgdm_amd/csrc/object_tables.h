// The 3-D objects of a guidance handle: their PointNet++ tables (ObjectTables) and the store that builds and owns them.
#pragma once
#include "common.h"
#include "models.h"
#include <memory>

namespace dgdm {

struct ObjectTables {       // 3-D, per object
    // slices of the store's pools (the FPS tables of all objects are built by one launch each)
    const float *xyz = nullptr;   // [N][3]
    const int   *fps1 = nullptr;  // [N][512]
    const int   *fps2 = nullptr;  // [N][128] FPS(128) sequence by start point
    const int   *flags = nullptr; // [N] that sequence is order-dependent (exact distance tie / coordinates exhausted)
    int    N = 0;
    DevBuf Z;               // [N][N][256]
    bool   fast_ok = false; // no flag set: rows can take their centres from fps2 instead of running FPS
    int *crowded = nullptr, *clist = nullptr;   // [N] int, [N + 1] int (clist[N] = count): centres whose ball query truncates (pointnet.hip crowd_kernel); pool slices
    DevBuf M0, cl2, cnt2;   // [N][256] float, [N][128] int, [N] int: variant-independent part of the sa3 max (pointnet.hip m0_kernel)
    DevBuf cl2s;            // [N][128] cl2 as positions in clist (xtab_kernel)
    DevBuf cl2o;            // [N][2][128] u16: cl2 as byte offsets into xobj_rows_kernel's LDS slab (scaled for the build's mode: has16), even / odd slots first
    DevBuf pcf;             // [N][512] per (s1, s2): sa2's start point, its list length, its tie flag (pointnet.hip pcf_kernel)
    DevBuf X, X16;          // [N][N][256] float32 / [N][N][128] bf16 dwords: the finished embedding per (s1, start point) (pointnet.hip xtab_kernel)
    bool   has_x = false, has_x16 = false;
    int    ncr = 0;         // number of crowded centres (read back: ObjectStore3D::finish)
    DevBuf Z16, M0_16;      // bf16 operand-order copies, built when the build's options say bf16
    bool   has16 = false;
    // [N][512] float, [N] int: layer 1's object part of the f16x3 trunk for the rows M0[q] - the scaled accumulators and the row's scale
    // exponent (trunk.h TrunkParams::l1z / l1k).  Written by the float32 build for an object without crowded centres (the
    // kernel looks at the device-side count); has_l1: the last build launched it, so the table is current whenever ncr == 0
    DevBuf L1Z, L1K;
    bool   has_l1 = false;
    // a chain of this object for the gather kernels (all but lpr, which depends on the launch's row format), and the object for xtab_kernel
    void fill(XobjChain *c) const;
    void fill(XtabObj *o) const;
};

// What a build does, decided by the handle's mode and test hooks at the time of the call
struct BuildOptions {
    bool bf16 = false;          // bf16 operand-order tables beside the float32 ones (the sa3 contraction on the bf16 matrix pipe)
    bool l2_gather = false;     // test hook: the sa2 features of the crowded centres by l2_kernel's global gathers (dense build)
    bool eager_xtab = false;    // the embedding tables right away (test hook; otherwise build_xtab, when the objects are being reused)
    bool l1tab = true;          // the layer-1 tables of the f16x3 gradient trunk (float32 build, N >= 128)
    bool off_stream = false;    // on the build streams alone: only the copy of the coordinates stays on the caller's stream
};

// Owns the tables of the handle's objects, the pools they are cut from, the build's temporaries, streams, events and read-back.
//
// Ordering rules, all of them kept here:
//  - `pooled` (caller's stream): the coordinates are in the pool, behind everything the caller enqueued before.  Every build stream
//    waits for it - and, off the caller's stream, for the previous build's end - before it overwrites pools or tables.
//  - `bstart` (FPS stream): the FPS tables exist.  `ldone` (build stream 0): the batched light stages' outputs exist, `crowd_ev` the
//    crowded-centre counts, the first of them.  The heavy per-object stages wait for bstart and ldone; odone[i] is recorded behind
//    object i's last heavy stage, so a stream that waits for it has the pool's parts of the object too (object_done).
//  - the read-back of the tie flags and crowded counts lands in pinned memory behind ro.ev and is waited for by finish() alone; a
//    build off the caller's stream enqueues it early (behind bstart and crowd_ev), in front of the heavy stages.
//  - `end`: the END of the build, behind every build stream, the layer-1 tables and the read-back.  join(s) makes a stream wait for
//    it; a reader of the tables joins first, or waits for tables_started / object_done where those cover what it reads.  The next
//    build and the destructor order themselves by the end of the build, never by the read-back.
//  - the destructor's body synchronises the build streams before any member is released: a build nobody joined may still be writing
//    the buffers.  A handle declares its store last, so that this happens before the handle's other buffers go as well (the
//    first build stream also runs work of the handle: first_stream).
class ObjectStore3D {
public:
    static constexpr int NBUILD = 3;             // most objects whose tables are built concurrently (own stream + 0.5 GB of temporaries each)
    ObjectStore3D() = default;
    ObjectStore3D(const ObjectStore3D &) = delete;
    ObjectStore3D &operator=(const ObjectStore3D &) = delete;
    ~ObjectStore3D();
    void init(DgdmDynamics *model, int num_object_points, int max_objects) { m = model; N = num_object_points; max_obj = max_objects > 1 ? max_objects : 1; }
    // the tables of objects_dev [n_objects][N][3], enqueued; `s`: the caller's stream
    int build(const float *objects_dev, int n_objects, const BuildOptions &o, hipStream_t s);
    int finish();                                // the host waits for the read-back of the last build: fast_ok and ncr of its objects are valid
    int join(hipStream_t s);                     // `s` waits for the build's end, unless it has (nothing is enqueued then)
    // a build off the caller's stream has still to be joined by `s`: its gathers may start object by object
    bool gather_early(hipStream_t s) const { return built_off_stream && (join_pending || s != joined_stream); }
    int tables_started(hipStream_t s) { return bstart.wait(s); }            // `s` waits for the FPS tables (what the index kernel reads)
    int object_done(int i, hipStream_t s) { return odone[i]->wait(s); }     // `s` waits for object i's tables
    // T8: the embedding table of object i in the format the trunk of the object's build mode reads (float32 for the parity path, bf16
    // operand-order rows when the object was built in bf16 mode); reads the finished tables (join first)
    int build_xtab(int i, hipStream_t s);
    const ObjectTables &operator[](int i) const { return *tables[i]; }
    int size() const { return n_objects; }       // objects of the last build
    int first_stream(hipStream_t *out) { return bstream[0].get(out); }      // idle once the build has been joined: the denoise loop's side stream

private:
    int build_object(int oi, int slot, const BuildOptions &o, hipStream_t s);
    DgdmDynamics *m = nullptr;
    int N = 0, max_obj = 1, n_objects = 0;
    std::vector<std::unique_ptr<ObjectTables>> tables;
    DevBuf pool_crowded, pool_clist, pool_off, pool_pairs, pool_rank, pool_F1, pool_U;   // [n_objects] x the light build stages' outputs (built by one launch per stage)
    DevBuf pool_xyz, pool_fps1, pool_fps2, pool_flags, pool_ncr;   // [n_objects] x per-object FPS tables (ObjectTables point into these), crowded-centre counts
    DevBuf pool_fps1t;                              // float32 build: [n_objects] x fps1 by position [64][N] x 16 B (l2sel_kernel reads it with the variants on its lanes)
    DevBuf tmpY[NBUILD], tmpL2[NBUILD], vlist;      // table-build temporaries of the heavy stages (per build stream)
    DevBuf tmpShare[NBUILD];                        // float32 build: the selection stage's outputs (pointnet.h L2Share), carved out of one buffer
    DevBuf l1objs;                                  // the layer-1 build's per-object pointer arrays [M0 | L1Z | L1K][max_objects]
    Stream bstream[NBUILD];
    Event bev[NBUILD], bstart, pooled, ldone, crowd_ev, end;
    std::vector<std::unique_ptr<Event>> odone;      // created once, re-recorded by every build
    PinnedBuf ro;                                   // [n_objects][N] tie flags, [n_objects] crowded counts; ro.ev: the copy has landed
    bool ro_pending = false;
    bool built_off_stream = false, join_pending = false;
    hipStream_t joined_stream = nullptr;
};

}  // namespace dgdm
