// RowEmbedder: draws -> embeddings for the rows of the 3-D classifier calls (row_embed.h has the ordering rules).
#include "row_embed.h"
#include "row_plan.h"
#include <algorithm>

namespace dgdm {

int RowEmbedder::init(int num_object_points, int64_t sub_batch_size, int nc, int64_t R) {
    N = num_object_points; sub_batch = sub_batch_size; max_chains = nc;
    int rc;
    if ((rc = starts.alloc((size_t)nc * R * 2 * sizeof(int))) ||
        (rc = order.alloc((size_t)nc * R * sizeof(int))) || (rc = xchains.alloc(sizeof(XobjChain) * nc)) ||
        (rc = todo.alloc(((size_t)nc * R + 1) * sizeof(int))))
        return rc;
    todo_capacity = (int64_t)nc * R;
    if ((rc = groupoff.alloc((size_t)nc * (N + 1) * sizeof(int))) || (rc = xidx.alloc((size_t)nc * R * sizeof(int))) ||
        (rc = xidxchains.alloc(sizeof(XidxChain) * nc)) || (rc = xtabptrs.alloc(sizeof(void *) * nc)) ||
        (rc = l1ptrs.alloc(sizeof(void *) * 3 * nc)))
        return rc;
    return staging.reserve(((size_t)nc * R * 3 + (size_t)nc * (N + 1)) * sizeof(int));
}

int RowEmbedder::ensure_rows(int n_chains, int64_t rows_per_chain) {
    const size_t nr = (size_t)n_chains * rows_per_chain;
    int rc;
    // (the embedding rows themselves - xobj / xobj16, 1 KiB / 512 B per row - are allocated by run_xobj, the only path that writes them:
    // with the embedding tables X[s1][q] in place a call gathers nothing)
    if ((rc = starts.alloc(nr * 2 * sizeof(int))) || (rc = order.alloc(nr * sizeof(int))) ||
        (rc = todo.alloc((nr + 1) * sizeof(int))) || (rc = xidx.alloc(nr * sizeof(int))))
        return rc;
    todo_capacity = (int64_t)nr;
    return staging.reserve((nr * 3 + (size_t)n_chains * (N + 1)) * sizeof(int));
}

int RowEmbedder::upload_starts(const int64_t *starts_host, int n_chains, int64_t rows, hipStream_t s, bool need_order, int n_calls,
                               int64_t call_stride, bool on_launch_stream) {
    const int64_t rt = rows * n_calls;                         // rows per chain on the device
    int rc;
    if ((rc = check_row_plan(rt, need_order)) || (rc = ensure_rows(n_chains, rt))) return rc;
    if ((rc = staging.ev.synchronize())) return rc;            // previous copy out of the staging buffer has finished
    int *dst = staging.as<int>();
    int *ord = dst + (size_t)n_chains * 2 * rt;
    int *goff = ord + (size_t)n_chains * rt;                   // [n_chains][N+1]
    if ((rc = plan_chain_rows(starts_host, n_chains, rows, n_calls, call_stride, sub_batch, N, need_order, dst, ord, goff))) return rc;
    hipStream_t cs;
    if ((rc = cstream.get(&cs))) return rc;
    // the copy may start as soon as the previous readers of the device buffers (the last gather / index kernel on the launch stream)
    // are done - not behind everything queued on the launch stream since.
    // on_launch_stream (the gathers start beside a table build still in flight, run_xobj): the copies go on `s` itself.  The process
    // has more streams than hardware queues, and up_ready's marker on the upload stream was seen to come out only behind the LAST
    // kernel of the build stream whose queue it shares - the gathers then started at the build's end whatever they waited for
    // (DESIGN.md 4.3b).  `s` has nothing else to run until the build ends, so the copy costs the gathers' start, not the step.
    hipStream_t us = on_launch_stream ? s : cs;
    if ((rc = up_consumed.wait(us))) return rc;
    if (need_order) {         // what the gathers read first
        DGDM_HIP_CHECK(hipMemcpyAsync(order.p, ord, (size_t)n_chains * rt * sizeof(int), hipMemcpyHostToDevice, us));
        DGDM_HIP_CHECK(hipMemcpyAsync(groupoff.p, goff, (size_t)n_chains * (N + 1) * sizeof(int), hipMemcpyHostToDevice, us));
    }
    DGDM_HIP_CHECK(hipMemcpyAsync(starts.p, dst, (size_t)n_chains * rt * 2 * sizeof(int), hipMemcpyHostToDevice, us));
    if ((rc = staging.ev.record(us))) return rc;
    if (!on_launch_stream && ((rc = up_ready.record(cs)) || (rc = up_ready.wait(s)))) return rc;
    return DGDM_OK;
}

int RowEmbedder::fill_l1ptrs(const std::vector<const ObjectTables *> &of_chain, int *n_tabled, hipStream_t s) {
    const int nc = max_chains;
    std::vector<const void *> ptrs(3 * (size_t)nc, nullptr);                       // [L1Z | L1K][nc] pointers, then the chain list [nc] ints
    int *list = reinterpret_cast<int *>(ptrs.data() + 2 * (size_t)nc);
    std::vector<int> rest;
    int nt = 0;
    for (size_t i = 0; i < of_chain.size(); ++i) {
        const ObjectTables *t = of_chain[i];
        if (!t || !l1tab || !t->has_l1 || t->ncr != 0) { rest.push_back((int)i); continue; }
        ptrs[i] = t->L1Z.p; ptrs[nc + i] = t->L1K.p;
        list[nt++] = (int)i;
    }
    std::copy(rest.begin(), rest.end(), list + nt);
    *n_tabled = nt;
    if (nt) DGDM_HIP_CHECK(hipMemcpyAsync(l1ptrs.p, ptrs.data(), sizeof(void *) * ptrs.size(), hipMemcpyHostToDevice, s));      // pageable: staged before return
    return DGDM_OK;
}

int RowEmbedder::index_rows(const std::vector<XidxChain> &xc, const std::vector<const void *> &base, const std::vector<const ObjectTables *> &m0_of,
                            bool l1_first, int64_t rows, int *l1, hipStream_t s) {
    const int n_chains = (int)xc.size();
    int rc;
    if (l1_first && (rc = fill_l1ptrs(m0_of, l1, s))) return rc;
    DGDM_HIP_CHECK(hipMemcpyAsync(xidxchains.p, xc.data(), sizeof(XidxChain) * n_chains, hipMemcpyHostToDevice, s));      // pageable: staged before return
    DGDM_HIP_CHECK(hipMemcpyAsync(xtabptrs.p, base.data(), sizeof(void *) * n_chains, hipMemcpyHostToDevice, s));
    if (!l1_first && (rc = fill_l1ptrs(m0_of, l1, s))) return rc;
    return pn_xidx(xidxchains.as<XidxChain>(), starts.as<int>(), rows, n_chains, xidx.as<int>(), s);
}

int RowEmbedder::use_xtab(const int *objidx_host, int n_chains, int64_t rows, bool want16, int *l1, hipStream_t s) {
    std::vector<XidxChain> xc(n_chains);
    std::vector<const void *> base(n_chains);
    std::vector<const ObjectTables *> m0_of(n_chains, nullptr);      // chains that read their object's float32 M0
    for (int i = 0; i < n_chains; ++i) {
        const ObjectTables &t = store[objidx_host[i]];
        xc[i].fps1 = t.fps1; xc[i].N = N; xc[i].m0_only = t.ncr == 0;
        // an object without crowded centres has X[s1][q] = M0[q]: its table is M0 itself (xtab_kernel wrote nothing)
        base[i] = want16 ? (t.ncr == 0 ? (const void *)t.M0_16.p : (const void *)t.X16.p) : (t.ncr == 0 ? (const void *)t.M0.p : (const void *)t.X.p);
        if (!want16 && t.ncr == 0) m0_of[i] = &t;
    }
    return index_rows(xc, base, m0_of, true, rows, l1, s);
}

int RowEmbedder::run_xobj(const int *objidx_host, int n_chains, int64_t rows, bool want16, bool trunk_bf16, bool *used16, bool *via_tab, int *l1,
                          hipStream_t s) {
    *via_tab = false;
    *l1 = 0;
    std::vector<XobjChain> ch(n_chains);
    for (int i = 0; i < n_chains; ++i) {
        const ObjectTables &t = store[objidx_host[i]];
        t.fill(&ch[i]);
        want16 = want16 && t.has16;          // bf16 rows only if every chain's object was built with its bf16 tables
    }
    {   // grow-only buffers (a run's embeds have the same size, or shrink at its tail: no reallocation under kernels in flight)
        const size_t nrows = (size_t)n_chains * rows;
        int rc = want16 ? xobj16.alloc(nrows * 512) : xobj.alloc(nrows * 256 * 4);
        if (rc) return rc;
    }
    *used16 = want16;
    XobjParams xp{};
    xp.chains = xchains.as<XobjChain>(); xp.starts = starts.as<int>(); xp.order = order.as<int>(); xp.xobj = xobj.as<float>();
    xp.xobj16 = want16 ? xobj16.as<uint32_t>() : nullptr;
    xp.R = rows; xp.total_rows = rows * n_chains; xp.use_table = force_slow_xobj ? 0 : 1;
    xp.todo = todo.as<int>(); xp.todo_count = todo.as<int>() + todo_capacity; xp.todo_capacity = todo_capacity;
    bool all_fast = true;
    for (int i = 0; i < n_chains; ++i) all_fast = all_fast && store[objidx_host[i]].fast_ok;
    // group kernel: every chain needs its tables and a slab chunk that fits LDS (it handles tie-flagged start points itself)
    bool groups = !force_slow_xobj && xobj_mode == 0 && N >= 128;
    for (int i = 0; i < n_chains && groups; ++i) {
        const ObjectTables &t = store[objidx_host[i]];
        ch[i].lpr = xobj_rows_lpr(t.ncr, want16);
        groups = ch[i].lpr > 0 && want16 == t.has16;     // the slot offsets are scaled for the build's mode
    }
    // only the group kernel's launches start ahead of the build's end (below); everything else reads the tables behind the join
    const bool early = groups && gather_early(s);
    if (!early) {
        int rc = store.join(s);
        if (rc) return rc;
    }
    DGDM_HIP_CHECK(hipMemcpyAsync(xchains.p, ch.data(), sizeof(XobjChain) * n_chains, hipMemcpyHostToDevice, s));     // pageable: staged before return
    if (!groups) return pn_xobj(xp, all_fast, s);
    // A chain whose object has no crowded centre and no tie-flagged start has M0[q] as the embedding of every row (use_xtab): it gets no
    // work items and its block of xobj is never written.  The trunk then reads EVERY chain of the launch through a table and a row
    // index: such a chain M0 at q = fps1[s1][s2], a gathered chain its own block of xobj at the row's number.  Not when the test hook
    // asks for materialised rows (modes 1-3), nor for the bf16 trunk on float32 rows (it has no float32 table form).
    const bool by_index = tables_wanted() && (want16 || !trunk_bf16);
    std::vector<int> rank;
    std::vector<XidxChain> xc(n_chains);
    std::vector<const void *> base(n_chains);
    std::vector<const ObjectTables *> m0_of(n_chains, nullptr);      // chains that read their object's float32 M0
    for (int i = 0; i < n_chains; ++i) {
        const ObjectTables &t = store[objidx_host[i]];
        const bool m0_only = by_index && t.ncr == 0 && t.fast_ok;
        if (!m0_only) rank.push_back(i);
        if (m0_only && !want16) m0_of[i] = &t;
        xc[i].fps1 = m0_only ? t.fps1 : nullptr; xc[i].N = N; xc[i].m0_only = 1;
        base[i] = m0_only ? (want16 ? (const void *)t.M0_16.p : (const void *)t.M0.p)
                          : (want16 ? (const void *)(xobj16.as<uint32_t>() + (size_t)i * rows * 128) : (const void *)(xobj.as<float>() + (size_t)i * rows * 256));
    }
    xp.group_off = groupoff.as<int>(); xp.nchain = n_chains; xp.group_N = N; xp.use_table = 1;
    auto index = [&]() -> int {
        *via_tab = true;
        return index_rows(xc, base, m0_of, false, rows, l1, s);
    };
    int rc;
    if (!early) {                        // one launch over all chains behind the joined build
        xp.total_items = (int)rank.size() * xp.group_N;
        std::stable_sort(rank.begin(), rank.end(), [&](int a, int b) { return ch[a].ncr > ch[b].ncr; });
        for (size_t i = 0; i < rank.size(); ++i) xp.chain_of_rank[i] = (unsigned char)rank[i];
        if ((rc = pn_xobj_groups(xp, s)) || !by_index) return rc;
        return index();
    }
    // Step schedule: the build is still running on its streams and `s` has not joined it.  A chain's rows are gathered
    // from its own object's tables alone, so they start behind that object's tables and run beside the float64 stages of the objects
    // still being built: one launch per object with gathered chains, in the order in which the builds end (object index order, round-
    // robin over the build streams).  All of them are on `s`, so what is recorded on `s` afterwards lies behind every gather:
    // up_consumed (embed_rows), the next build's `pooled` (it may overwrite tables and pool), the previous run's trunk that
    // read xobj lies in front.  The launches append to ONE list of tie-flagged rows, emptied once; those rows (they read the
    // tables of any chain), and the trunk's reads of M0 / L1Z, come behind store.join(s) - which is reached on every way out,
    // an error half way included, so that nothing enqueued here is left un-joined.
    auto gathers = [&]() -> int {
        int rc;
        if (by_index && ((rc = store.tables_started(s)) || (rc = index()))) return rc;      // the index kernel needs the FPS tables, nothing of the heavy stages
        if (rank.empty()) return DGDM_OK;
        if ((rc = pn_xobj_groups_begin(xp, s))) return rc;
        for (int o = 0; o < store.size(); ++o) {
            int n = 0;                   // (the chains of one object have the same ncr: no heaviest-first order within a launch)
            for (int c : rank)
                if (objidx_host[c] == o) xp.chain_of_rank[n++] = (unsigned char)c;
            if (!n) continue;
            xp.total_items = n * xp.group_N;
            if ((rc = store.object_done(o, s)) || (rc = pn_xobj_groups_rows(xp, s))) return rc;
        }
        return DGDM_OK;
    };
    rc = gathers();
    const int jrc = store.join(s);
    if (rc || jrc) return rc ? rc : jrc;
    return rank.empty() ? DGDM_OK : pn_xobj_groups_ties(xp, s);
}

int RowEmbedder::embed_rows(const int *oidx, int n_chains, const int64_t *starts_host, int64_t rows_per_call, int n_calls, int64_t call_stride,
                            bool want16, bool trunk_bf16, Embedded *e, hipStream_t s) {
    bool tab = tables_wanted();
    for (int i = 0; i < n_chains && tab; ++i) tab = want16 ? store[oidx[i]].has_x16 : store[oidx[i]].has_x;   // else: built in the other format, or not at all
    const int64_t rt = rows_per_call * n_calls;
    int rc;
    // Every reader of the tables joins the build in front of its first read: the embedding-table path here, run_xobj where its
    // kernels need the whole build (its per-object gathers start earlier, see there), DgdmGuidance::embed in front of a build_xtab.
    if (tab && (rc = store.join(s))) return rc;
    if ((rc = upload_starts(starts_host, n_chains, rows_per_call, s, !tab, n_calls, call_stride, !tab && gather_early(s)))) return rc;     // host work: overlaps a table build still in flight
    if ((rc = store.finish())) return rc;
    e->tab = tab; e->used16 = want16; e->rows_per_chain = rt;
    if ((rc = tab ? use_xtab(oidx, n_chains, rt, want16, &e->l1, s) : run_xobj(oidx, n_chains, rt, want16, trunk_bf16, &e->used16, &e->tab, &e->l1, s))) return rc;
    return up_consumed.record(s);            // the index buffers may be overwritten once these kernels are through
}

void Embedded::point(TrunkParams *p, const RowEmbedder &r, int call, int64_t rows_per_call) const {
    const size_t row0 = (size_t)call * rows_per_call;
    p->xstride = rows_per_chain;
    if (tab) {
        p->xidx = r.xidx.as<int>() + row0;
        if (used16) p->xtab16 = r.xtabptrs.as<const uint32_t *>();
        else p->xtab = r.xtabptrs.as<const float *>();
        if (l1 && !used16) {                     // read by the f16x3 gradient trunk alone
            p->l1z = r.l1ptrs.as<const float *>();
            p->l1k = r.l1ptrs.as<const int *>() + r.max_chains;
            p->chainlist = reinterpret_cast<const int *>(r.l1ptrs.as<const void *>() + 2 * (size_t)r.max_chains);
            p->n_tabled = l1;
        }
    } else {
        p->xobj = r.xobj.as<float>() + row0 * 256;
        p->xobj16 = used16 ? r.xobj16.as<uint32_t>() + row0 * 128 : nullptr;
    }
}

}  // namespace dgdm
