// ObjectStore3D: the PointNet++ tables of a guidance handle's 3-D objects and their build (object_tables.h has the ordering rules).
#include "object_tables.h"
#include <algorithm>

namespace dgdm {

void ObjectTables::fill(XobjChain *c) const {
    c->xyz = xyz; c->fps1 = fps1; c->slot_of_start = nullptr; c->Z = Z.as<float>();
    c->fps2 = fps2; c->flags = flags; c->crowded = crowded; c->N = N;
    c->M0 = M0.as<float>(); c->cl2 = cl2.as<int>(); c->cnt2 = cnt2.as<int>();
    c->Z16 = has16 ? Z16.as<uint32_t>() : nullptr; c->M0_16 = has16 ? M0_16.as<uint32_t>() : nullptr;
    c->clist = clist; c->cl2s = cl2s.as<int>(); c->cl2o = cl2o.as<unsigned short>(); c->pcf = pcf.as<int>(); c->ncr = ncr;
}

void ObjectTables::fill(XtabObj *o) const {
    o->xyz = xyz; o->fps1 = fps1; o->Z = Z.as<float>(); o->M0 = M0.as<float>();
    o->Z16 = has16 ? Z16.as<uint32_t>() : nullptr; o->M0_16 = has16 ? M0_16.as<uint32_t>() : nullptr;
    o->clist = clist; o->ncr = clist + N; o->cl2s = cl2s.as<int>(); o->cnt2 = cnt2.as<int>(); o->flags = flags;
    o->crowded = crowded; o->X = has16 ? nullptr : X.as<float>(); o->X16 = has16 ? X16.as<uint32_t>() : nullptr; o->N = N;
}

ObjectStore3D::~ObjectStore3D() {
    for (const Stream &b : bstream) b.synchronize();      // before any member goes (object_tables.h)
}

int ObjectStore3D::build_object(int oi, int slot, const BuildOptions &opt, hipStream_t s) {
    ObjectTables &t = *tables[oi];
    const bool bf16 = opt.bf16;
    const PnWeights w = m->pn();
    int rc;
    if ((rc = t.Z.alloc((size_t)N * N * 256 * 4)) ||
        (rc = t.M0.alloc((size_t)N * 256 * 4)) || (rc = t.cl2.alloc((size_t)N * 128 * sizeof(int))) || (rc = t.cnt2.alloc((size_t)N * sizeof(int))) ||
        (rc = t.cl2s.alloc((size_t)N * 128 * sizeof(int))) || (rc = t.cl2o.alloc((size_t)N * 256 * sizeof(unsigned short))) ||
        (rc = t.pcf.alloc((size_t)N * 512 * sizeof(int))))
        return rc;
    t.has16 = bf16;
    if (bf16 && ((rc = t.Z16.alloc((size_t)N * N * 128 * 4)) || (rc = t.M0_16.alloc((size_t)N * 128 * 4)))) return rc;
    uint32_t *z16 = bf16 ? t.Z16.as<uint32_t>() : nullptr;
    DevBuf &tY = tmpY[slot], &tL2 = tmpL2[slot];
    if ((rc = tY.alloc((size_t)N * N * 256 * 4)) || (rc = tL2.alloc((size_t)N * N * 256 * 4))) return rc;
    const float *xyz = t.xyz;                                                                                  // T1: build(), batched
    // crowded flags / pair lists (crowd_kernel, nbr_fill_kernel), T2 (sa1) and T3 (U): build(), one launch per stage for all objects
    const int *off = pool_off.as<int>() + (size_t)oi * (N + 1), *pairs = pool_pairs.as<int>() + (size_t)oi * N * N;
    const short *rank = pool_rank.as<short>() + (size_t)oi * N * N;
    const char *U = static_cast<const char *>(pool_U.p) + (size_t)oi * N * 128 * (bf16 ? 4 : 8);      // float32 rows in bf16 mode, float64 otherwise
    if (bf16) {
        // bf16 mode: the sa3 contraction (T6) runs on the bf16 matrix pipe and rounds its input, so T4 writes and T5 reduces bf16
        // rows (the temporaries tY / tL2 are simply used at half size); the stages in front of it stay float32
        if ((rc = pn_pairs(xyz, N, reinterpret_cast<const float *>(U), w, pairs, off, tY.as<float>(), tY.as<uint32_t>(), s))) return rc;   // T4
        if ((rc = pn_l2(xyz, N, w, t.fps1, vlist.as<int>(), N, tY.as<float>(), tL2.as<float>(), t.clist, t.clist + N,
                        off, rank, true, s, opt.l2_gather ? 0 : 1))) return rc;                    // T5
        if ((rc = pn_z16(xyz, N, N, w, tL2.as<uint32_t>(), t.Z.as<float>(), z16, t.clist, t.clist + N, s))) return rc;          // T6
    } else {
        // float32 mode (the parity path): every contraction of the build accumulates in float64 and each table entry is rounded once
        // (pointnet64.hip); the max stages (T5, T7) are exact as they are
        const PnWeights64 w64 = m->pn64();
        if ((rc = pn_pairs64(xyz, N, reinterpret_cast<const double *>(U), w64, pairs, off, tY.as<float>(), s))) return rc;                 // T4
        // T5 / T6 of the crowded centres once per DISTINCT first-64 selection: Z[v][c] depends on v only through which points of c's ball
        // come first in fps1[v], and many variants select the same set.  The test hook's dense build (l2_gather) and clouds the
        // crowded-centre kernel does not take (N > 512) compute every (variant, centre) row from its own L2 row.
        const bool shared = !opt.l2_gather && N <= 512;
        L2Share sh{};
        if (shared) {
            const size_t NN = (size_t)N * N;
            if ((rc = tmpShare[slot].alloc(NN * 64 + NN + NN * sizeof(short) + NN * sizeof(int) + (2 * (size_t)N + 4) * sizeof(int)))) return rc;
            char *b = static_cast<char *>(tmpShare[slot].p);
            sh.sel = reinterpret_cast<unsigned char *>(b); b += NN * 64;
            sh.items = reinterpret_cast<int *>(b); b += NN * sizeof(int);
            sh.coff = reinterpret_cast<int *>(b); b += N * sizeof(int);
            sh.ccnt = reinterpret_cast<int *>(b); b += N * sizeof(int);
            sh.nitems = reinterpret_cast<int *>(b); b += 4 * sizeof(int);
            sh.rep = reinterpret_cast<short *>(b); b += NN * sizeof(short);
            sh.cnt = reinterpret_cast<unsigned char *>(b);
            sh.fps1t = pool_fps1t.as<uint4>() + (size_t)oi * N * 64;
        }
        if ((rc = pn_l2(xyz, N, w, t.fps1, vlist.as<int>(), N, tY.as<float>(), tL2.as<float>(), t.clist, t.clist + N,
                        off, rank, false, s, shared ? 1 : 0, shared ? &sh : nullptr))) return rc;  // T5
        if ((rc = pn_z64(xyz, N, N, w64, tL2.as<float>(), t.Z.as<float>(), t.clist, t.clist + N, s, sh.items, sh.nitems))) return rc;   // T6
        if (shared && N > 1 && (rc = pn_zfill(N, N, t.Z.as<float>(), t.clist, t.clist + N, sh.rep, s))) return rc;
    }
    if ((rc = pn_m0(t.fps2, t.crowded, N, t.Z.as<float>(), t.M0.as<float>(), t.cl2.as<int>(), t.cnt2.as<int>(), z16,
                    bf16 ? t.M0_16.as<uint32_t>() : nullptr, t.clist, t.clist + N, t.cl2s.as<int>(), t.cl2o.as<unsigned short>(), s))) return rc;          // T7
    if ((rc = pn_pcf(t.fps1, t.cnt2.as<int>(), t.flags, N, t.pcf.as<int>(), s))) return rc;
    t.has_x = t.has_x16 = false;
    return opt.eager_xtab ? build_xtab(oi, s) : DGDM_OK;       // eager only on request: DgdmGuidance::embed has when it pays
}

int ObjectStore3D::build_xtab(int oi, hipStream_t s) {
    ObjectTables &t = *tables[oi];
    if (N < 128) return DGDM_OK;
    const bool b16 = t.has16;
    int rc;
    if (b16) { if ((rc = t.X16.alloc((size_t)N * N * 128 * 4))) return rc; }
    else if ((rc = t.X.alloc((size_t)N * N * 256 * 4))) return rc;
    XtabObj xo{};
    t.fill(&xo);
    if ((rc = pn_xtab(xo, b16, s))) return rc;
    (b16 ? t.has_x16 : t.has_x) = true;
    return DGDM_OK;
}

int ObjectStore3D::build(const float *objects_dev, int n_obj, const BuildOptions &opt, hipStream_t s) {
    int rc;
    prof_begin(s, DGDM_STAGE_TABLES);
    while ((int)tables.size() < n_obj) tables.emplace_back(new ObjectTables());
    if (vlist.bytes < (size_t)N * sizeof(int)) {
        std::vector<int> v(N);
        for (int i = 0; i < N; ++i) v[i] = i;
        if ((rc = vlist.upload(v.data(), sizeof(int) * N))) return rc;
    }
    // objects are independent: build them round-robin on a few side streams so the latency-bound stages (FPS: 512
    // dependent iterations on 128 workgroups) of one object overlap the bandwidth/MFMA-bound stages of the others
    const int nb = std::min<int>(NBUILD, n_obj);
    // off the caller's stream (step schedule): only the copy of the coordinates stays on `s`; the FPS tables go to
    // the last build stream (a second one even for a single object: they run beside the light stages), and what reads the tables
    // later waits for the build's end (join)
    const bool off = opt.off_stream, bf16 = opt.bf16;
    const int ns = off ? std::max(nb, 2) : nb;
    if (!off && (rc = join(s))) return rc;      // an earlier build off this stream that nobody has joined yet
    hipStream_t bs[NBUILD] = {};
    for (int i = 0; i < ns; ++i)
        if ((rc = bstream[i].get(&bs[i]))) return rc;
    // T1 for every object at once (stream `fs` below): fps1[obj][start][512], fps2[obj][start point][128] + tie flags
    const size_t no = (size_t)n_obj;
    if ((rc = pool_xyz.alloc(no * N * 3 * 4)) || (rc = pool_fps1.alloc(no * N * 512 * sizeof(int))) ||
        (rc = pool_fps2.alloc(no * N * 128 * sizeof(int))) || (rc = pool_flags.alloc(no * N * sizeof(int))) ||
        (rc = pool_ncr.alloc(no * sizeof(int))) || (rc = pool_crowded.alloc(no * N * sizeof(int))) ||
        (rc = pool_clist.alloc(no * (N + 1) * sizeof(int))) || (rc = pool_off.alloc(no * (N + 1) * sizeof(int))) ||
        (rc = pool_pairs.alloc(no * N * N * sizeof(int))) || (rc = pool_rank.alloc(no * N * N * sizeof(short))) ||
        (rc = pool_F1.alloc(no * N * 128 * 8)) || (rc = pool_U.alloc(no * N * 128 * 8)) ||
        (rc = pool_fps1t.alloc(no * N * 64 * sizeof(uint4))))
        return rc;
    // the layer-1 tables of the f16x3 gradient trunk (built at the end, below): the float32 build's, for clouds the M0-only path serves.
    // Their pointer arrays [M0 | L1Z | L1K][max_objects] go up in front of `pooled`, which every build stream waits for (the buffers
    // never move - N and max_objects are the handle's - so a build still in flight reads the same values)
    const bool l1 = opt.l1tab && !bf16 && N >= 128;
    const size_t l1mo = (size_t)max_obj;
    if (l1) {
        std::vector<const void *> ptrs(3 * l1mo, nullptr);
        for (int i = 0; i < (int)tables.size(); ++i) {
            ObjectTables &t = *tables[i];
            if ((rc = t.M0.alloc((size_t)N * 256 * 4)) || (rc = t.L1Z.alloc((size_t)N * 512 * 4)) || (rc = t.L1K.alloc((size_t)N * sizeof(int)))) return rc;
            ptrs[i] = t.M0.p; ptrs[l1mo + i] = t.L1Z.p; ptrs[2 * l1mo + i] = t.L1K.p;
        }
        if ((rc = l1objs.alloc(sizeof(void *) * ptrs.size()))) return rc;
        DGDM_HIP_CHECK(hipMemcpyAsync(l1objs.p, ptrs.data(), sizeof(void *) * ptrs.size(), hipMemcpyHostToDevice, s));      // pageable: staged before return
    }
    for (int i = 0; i < n_obj; ++i) tables[i]->has_l1 = l1;
    DGDM_HIP_CHECK(hipMemcpyAsync(pool_xyz.p, objects_dev, no * N * 3 * 4, hipMemcpyDeviceToDevice, s));
    if ((rc = pooled.record(s))) return rc;
    hipStream_t fs = s;
    if (off) {
        // `pooled` lies behind everything the previous chains enqueued on `s` (their side-stream work is joined into `s` before
        // they return), so the build may overwrite the tables they read; a previous build nobody joined has ended at `end`
        fs = bs[ns - 1];
        for (int i = 1; i < ns; ++i)
            if ((rc = pooled.wait(bs[i])) || (rc = end.wait(bs[i]))) return rc;
    }
    // sa2's FPS table is the first 128 columns of sa1's (same clouds, same starts): one pass writes both and the tie flags
    if ((rc = pn_fps_tables(pool_xyz.as<float>(), N, N, pool_fps1.as<int>(), pool_fps2.as<int>(), pool_flags.as<int>(), fs, n_obj)))
        return rc;
    // the float32 build's selection stage reads the table by position (variants on its lanes): a transposed copy behind it
    if (!bf16 && !opt.l2_gather && N <= 512 &&
        (rc = pn_fps_transpose(pool_fps1.as<int>(), N, pool_fps1t.as<uint4>(), fs, n_obj))) return rc;
    if ((rc = bstart.record(fs))) return rc;
    // per-object completion events and the pinned target of the read-back (a copy of an earlier build into the old block has landed
    // at ro.ev before the block goes)
    while ((int)odone.size() < n_obj) odone.emplace_back(new Event());
    if ((rc = ro.reserve((no * N + no) * sizeof(int)))) return rc;
    for (int i = 0; i < n_obj; ++i) {
        ObjectTables &t = *tables[i];
        t.N = N;
        t.xyz = pool_xyz.as<float>() + (size_t)i * N * 3; t.fps1 = pool_fps1.as<int>() + (size_t)i * N * 512;
        t.fps2 = pool_fps2.as<int>() + (size_t)i * N * 128; t.flags = pool_flags.as<int>() + (size_t)i * N;
        t.crowded = pool_crowded.as<int>() + (size_t)i * N; t.clist = pool_clist.as<int>() + (size_t)i * (N + 1);
    }
    // the light, latency-bound stages - crowded flags + pair lists, T2 (sa1 features), T3 (U = sa2's first layer on the features) -
    // for ALL objects in one launch each (per object they are 1 .. 512 small workgroups: 130-500 us of a build stream each, a third
    // of its time), on the first build stream, beside the FPS tables; the heavy per-object stages (T4 .. T7) follow on the build streams
    {
        hipStream_t ls = bs[0];
        if ((rc = pooled.wait(ls))) return rc;          // the objects' coordinates are in the pool
        const PnWeights w = m->pn();
        if ((rc = pn_crowd(pool_xyz.as<float>(), N, w, pool_crowded.as<int>(), pool_clist.as<int>(), pool_clist.as<int>() + N,
                           pool_off.as<int>(), pool_pairs.as<int>(), pool_rank.as<short>(), ls, pool_ncr.as<int>(), n_obj)))
            return rc;
        if ((rc = crowd_ev.record(ls))) return rc;      // the crowded-centre counts exist
        if (bf16) {
            if ((rc = pn_sa1(pool_xyz.as<float>(), N, w, pool_F1.as<float>(), ls, n_obj))) return rc;                                   // T2
            if ((rc = linear(pool_F1.as<float>(), 128, w.sa2_wf_t, w.sa2_b0, nullptr, 1, pool_U.as<float>(), 128, n_obj * N, 128, 128,
                             ACT_NONE, false, ls))) return rc;                                                                           // T3
        } else {
            const PnWeights64 w64 = m->pn64();
            if ((rc = pn_sa1_64(pool_xyz.as<float>(), N, w.r1sq, w64, pool_F1.as<double>(), ls, n_obj))) return rc;                      // T2
            if ((rc = linear64(nullptr, pool_F1.as<double>(), 128, w64.sa2_wf_t, w64.sa2_b0, nullptr, 1, pool_U.as<double>(), nullptr, 128,
                               n_obj * N, 128, 128, ACT_NONE, ls))) return rc;                                                           // T3
        }
        if ((rc = ldone.record(ls))) return rc;
    }
    // which objects may use the table of FPS(128) sequences (no order-dependent selection anywhere); crowded-centre counts: copied
    // to pinned memory behind ro.ev, read by finish() when first needed.  Off the caller's stream they go as soon as both
    // exist: on the FPS stream right behind the tables (pool_flags) and behind the first light stage (pool_ncr), in front of that
    // stream's heavy stages - the host can plan the chains' gathers while those run
    auto read_back = [&](hipStream_t rs) -> int {
        DGDM_HIP_CHECK(hipMemcpyAsync(ro.as<int>(), pool_flags.p, sizeof(int) * no * N, hipMemcpyDeviceToHost, rs));
        DGDM_HIP_CHECK(hipMemcpyAsync(ro.as<int>() + no * N, pool_ncr.p, sizeof(int) * no, hipMemcpyDeviceToHost, rs));
        return ro.ev.record(rs);
    };
    if (off && ((rc = crowd_ev.wait(fs)) || (rc = read_back(fs)))) return rc;
    for (int i = 0; i < nb; ++i)         // the heavy stages need the FPS tables (bstart) and the light stages' outputs
        if ((rc = bstart.wait(bs[i])) || (rc = ldone.wait(bs[i]))) return rc;
    for (int i = 0; i < n_obj; ++i) {
        // behind the object's last stage its tables are complete: the gather of its chains' rows may start (object_done).  The stream
        // waited for bstart and ldone, so the pool's parts of the object (fps1, clist, ..) are covered too
        if ((rc = build_object(i, i % nb, opt, bs[i % nb])) || (rc = odone[i]->record(bs[i % nb]))) return rc;
    }
    // the build's end: on the caller's stream, or (off it) on build stream 0, which has the FPS stream behind it through bstart
    hipStream_t es = off ? bs[0] : s;
    for (int i = off ? 1 : 0; i < nb; ++i)
        if ((rc = bev[i].record(bs[i])) || (rc = bev[i].wait(es))) return rc;
    // every object's M0 and crowded count exist: the layer-1 tables of the uncrowded ones, all objects in one launch (in front of
    // `end`: join covers it)
    if (l1) {
        void *const *po = l1objs.as<void *>();
        if ((rc = trunk_f16l_l1_tables(reinterpret_cast<const float *const *>(po), pool_ncr.as<int>(), reinterpret_cast<float *const *>(po + l1mo),
                                       reinterpret_cast<int *const *>(po + 2 * l1mo), N, n_obj, m->fwdh(), es))) return rc;
    }
    prof_end(s, DGDM_STAGE_TABLES, 0.0);         // the stage's events bracket the build, not the read-back
    if (!off && (rc = read_back(es))) return rc;
    // `end` has the early read-back behind it as well (long complete by then): the next build's, possibly on another stream, cannot
    // overtake it
    if (off && (rc = ro.ev.wait(es))) return rc;
    if ((rc = end.record(es))) return rc;
    n_objects = n_obj;
    ro_pending = true;
    built_off_stream = off; join_pending = off;
    return DGDM_OK;
}

int ObjectStore3D::finish() {
    if (!ro_pending) return DGDM_OK;
    int rc = ro.ev.synchronize();                // the read-back alone: the build may still be running
    if (rc) return rc;
    const int *host = ro.as<int>();
    for (int i = 0; i < n_objects; ++i) {
        bool ok = N >= 128;
        for (int k = 0; k < N; ++k) ok = ok && host[(size_t)i * N + k] == 0;
        tables[i]->fast_ok = ok;
        tables[i]->ncr = host[(size_t)n_objects * N + i];
    }
    ro_pending = false;
    return DGDM_OK;
}

int ObjectStore3D::join(hipStream_t s) {
    if (!gather_early(s)) return DGDM_OK;
    int rc = end.wait(s);
    if (rc) return rc;
    join_pending = false; joined_stream = s;
    return DGDM_OK;
}

}  // namespace dgdm
