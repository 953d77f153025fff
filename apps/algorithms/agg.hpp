// Neighbour aggregation (`agg`): the fused HIP path (vgl_hip_agg_*, the contract of include/vgl_hip.h) over a stored direction of the graph and a
// sequential host restatement of the same contract in float64 for -check.  The reference has no counterpart.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

struct NeighbourAggregation {
    struct Options { int features = 64, op = VGL_HIP_AGG_SUM; bool weighted = false, outgoing = false, backward = false; };
    // what a run leaves on the host: out (rows x F) and, for max / min, arg; with -backward gx (V x F) of the gradient g
    struct Result { std::vector<float> out, gx; std::vector<int> arg; vgl_hip_agg_stats st, st_back; };

    // x, g (V x F) and w (one per entry) on the device: a counter hash of the position, the generator of the sssp weights
    struct Inputs {
        void *x = nullptr, *g = nullptr, *w = nullptr;
        size_t V = 0, E = 0, F = 0;
        Inputs(VGL_Graph &graph, const vgl_csr_view &view, const Options &o, unsigned long long seed) : V((size_t)graph.get_vertices_count()), E((size_t)view.edges), F((size_t)o.features)
        {
            vgl_hip_ctx *c = VGL_RUNTIME::ctx();
            VGL_HIP_CALL(vgl_hip_malloc(c, sizeof(float) * std::max<size_t>(V * F, 1), &x));
            VGL_HIP_CALL(vgl_hip_malloc(c, sizeof(float) * std::max<size_t>(V * F, 1), &g));
            VGL_HIP_CALL(vgl_hip_malloc(c, sizeof(float) * std::max<size_t>(E, 1), &w));
            VGL_HIP_CALL(vgl_hip_gen_weights(c, 0, (int64_t)(V * F), seed, (float *)x));
            VGL_HIP_CALL(vgl_hip_gen_weights(c, 0, (int64_t)(V * F), seed + 2, (float *)g));
            VGL_HIP_CALL(vgl_hip_gen_weights(c, 0, (int64_t)E, seed + 1, (float *)w));
            VGL_HIP_CALL(vgl_hip_ctx_sync(c));
        }
        ~Inputs()
        {
            vgl_hip_ctx *c = VGL_RUNTIME::ctx();
            vgl_hip_free(c, x); vgl_hip_free(c, g); vgl_hip_free(c, w);
        }
        std::vector<float> host(const void *d, size_t n) const
        {
            std::vector<float> h(n);
            if (n) VGL_HIP_CALL(vgl_hip_memcpy_d2h(VGL_RUNTIME::ctx(), h.data(), d, sizeof(float) * n));
            return h;
        }
    };

    static void print_stats(const char *what, const vgl_hip_agg_stats &s, double seconds)
    {
        std::cout << what << ": rows " << s.rows << ", entries " << s.entries << ", rows short / wave / wg " << s.rows_short << " / " << s.rows_wave << " / " << s.rows_wg << ", chunks "
                  << s.chunks << ", hub rows " << s.hub_rows << ", column tiles " << s.column_tiles[0] << " / " << s.column_tiles[1] << " / " << s.column_tiles[2] << ", vec " << s.vec
                  << ", transposed " << s.transposed << ", " << s.algorithmic_bytes << " bytes of the model, " << seconds * 1000.0 << " ms, " << s.algorithmic_bytes / (seconds * 1e9)
                  << " GB/s" << std::endl;
    }

    // plan (timed), a heat run, a timed run; with -backward the first transposed run (it builds the transpose) and a timed one.  Returns MTEPS.
    static double hip_fused(const vgl_csr_view &view, const Inputs &in, const Options &o, Result &r, bool launches = false)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        const size_t V = in.V, F = in.F;
        const bool ext = o.op == VGL_HIP_AGG_MAX || o.op == VGL_HIP_AGG_MIN;
        const float *w = o.weighted ? (const float *)in.w : nullptr;
        void *d_out = nullptr, *d_arg = nullptr, *d_gx = nullptr;
        VGL_HIP_CALL(vgl_hip_malloc(c, sizeof(float) * std::max<size_t>(V * F, 1), &d_out));
        VGL_HIP_CALL(vgl_hip_malloc(c, sizeof(int) * std::max<size_t>(V * F, 1), &d_arg));
        VGL_HIP_CALL(vgl_hip_malloc(c, sizeof(float) * std::max<size_t>(V * F, 1), &d_gx));
        vgl_hip_agg_plan *plan = nullptr;
        Timer prep, tm, first, back;
        prep.start();
        VGL_HIP_CALL(vgl_hip_agg_plan_create(c, (const int64_t *)view.rowptr, (const int32_t *)view.adj, (int32_t)V, (int32_t)V, &plan));
        prep.end();
        int32_t *arg = ext ? (int32_t *)d_arg : nullptr;
        VGL_HIP_CALL(vgl_hip_agg_run(c, plan, o.op, w, (const float *)in.x, (int64_t)F, (int32_t)F, (float *)d_out, (int64_t)F, arg, &r.st));      // heat run
        tm.start();
        VGL_HIP_CALL(vgl_hip_agg_run(c, plan, o.op, w, (const float *)in.x, (int64_t)F, (int32_t)F, (float *)d_out, (int64_t)F, arg, &r.st));
        tm.end();
        double seconds = tm.get_time();
        if (!launches) {
            std::cout << "AGG plan: " << prep.get_time() * 1000.0 << " ms" << std::endl;
            print_stats("AGG forward", r.st, seconds);
        }
        if (o.backward) {
            first.start();
            VGL_HIP_CALL(vgl_hip_agg_run_transposed(c, plan, o.op, w, arg, (const float *)in.g, (int64_t)F, (int32_t)F, (float *)d_gx, (int64_t)F, &r.st_back));
            first.end();
            back.start();
            VGL_HIP_CALL(vgl_hip_agg_run_transposed(c, plan, o.op, w, arg, (const float *)in.g, (int64_t)F, (int32_t)F, (float *)d_gx, (int64_t)F, &r.st_back));
            back.end();
            if (!launches) {
                std::cout << "AGG transpose: " << (first.get_time() - back.get_time()) * 1000.0 << " ms (the first backward run less a later one)" << std::endl;
                print_stats("AGG backward", r.st_back, back.get_time());
            }
            seconds += back.get_time();
        }
        if (!launches) {
            r.out = in.host(d_out, V * F);
            if (ext) { r.arg.resize(V * F); if (V * F) VGL_HIP_CALL(vgl_hip_memcpy_d2h(c, r.arg.data(), d_arg, sizeof(int) * V * F)); }
            if (o.backward) r.gx = in.host(d_gx, V * F);
        }
        VGL_HIP_CALL(vgl_hip_agg_plan_destroy(c, plan));
        VGL_HIP_CALL(vgl_hip_free(c, d_out));
        VGL_HIP_CALL(vgl_hip_free(c, d_arg));
        VGL_HIP_CALL(vgl_hip_free(c, d_gx));
        if (launches) return 0.0;
        const long long walked = (long long)r.st.entries * (o.backward ? 2 : 1);
        performance_stats.print_algorithm_performance_stats("AGG (fused)", seconds, walked);
        return performance_stats.get_algorithm_performance(seconds, walked);
    }

    // launches per timing slot of one more (untimed) plan and run with the event brackets on
    static void print_launches(const vgl_csr_view &view, const Inputs &in, const Options &o)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        Result r;
        VGL_HIP_CALL(vgl_hip_timing_reset(c));
        VGL_HIP_CALL(vgl_hip_timing_enable(c, 1));
        hip_fused(view, in, o, r, true);
        int64_t total = 0;
        std::cout << "AGG launches:";
        for (const char *name : {"agg_prepare", "agg_transpose", "agg_short", "agg_wave", "agg_wg", "agg_hubs"}) {
            int64_t n = 0;
            double ms = 0.0;
            VGL_HIP_CALL(vgl_hip_timing_get(c, name, &n, &ms));
            std::cout << " " << name << " " << n << " (" << ms << " ms)";
            total += n;
        }
        std::cout << ", total " << total << std::endl;
        VGL_HIP_CALL(vgl_hip_timing_enable(c, 0));
    }

    // gamma_k at u = 2^-24 plus the host's own at u = 2^-53, k = d + 2
    static double tolerance(long long d)
    {
        const double k = (double)(d + 2), u32 = std::ldexp(1.0, -24), u64 = std::ldexp(1.0, -53);
        return k * u32 / (1.0 - k * u32) + k * u64 / (1.0 - k * u64);
    }

    // the contract on the host in float64, entry by entry, against what the device left; the arg for equality
    static int verify(const HostCSR &h, const Inputs &in, const Options &o, const Result &r)
    {
        const size_t V = in.V, F = in.F;
        const bool ext = o.op == VGL_HIP_AGG_MAX || o.op == VGL_HIP_AGG_MIN, mean = o.op == VGL_HIP_AGG_MEAN;
        const double sign = o.op == VGL_HIP_AGG_MIN ? -1.0 : 1.0;
        const std::vector<float> x = in.host(in.x, V * F), g = in.host(in.g, V * F), w = in.host(in.w, in.E);
        int errors = 0;
        double worst = 0.0;
        auto judge = [&](const char *what, size_t at, double got, double want, double mag, long long d) {
            const double bound = tolerance(d) * mag, err = std::fabs(got - want);
            if (bound > 0.0) worst = std::max(worst, err / bound);
            if (!(err <= bound) && errors++ < 10) std::cout << "error in " << what << " at " << at << ": " << got << " vs " << want << " (bound " << bound << ")" << std::endl;
        };
        Timer host;
        host.start();
        std::vector<double> acc(F), mag(F);
        std::vector<long long> pos(F);
        for (size_t i = 0; i < V; i++) {
            const long long lo = h.rowptr[i], hi = h.rowptr[i + 1], len = hi - lo;
            std::fill(acc.begin(), acc.end(), 0.0); std::fill(mag.begin(), mag.end(), 0.0); std::fill(pos.begin(), pos.end(), -1LL);
            for (long long p = lo; p < hi; p++) {
                const float *row = x.data() + (size_t)h.adj[(size_t)p] * F;
                const double cf = o.weighted ? (double)w[(size_t)p] : 1.0;
                for (size_t f = 0; f < F; f++) {
                    if (ext) { if (pos[f] < 0 || sign * row[f] > acc[f]) { acc[f] = sign * row[f]; pos[f] = p; } }
                    else { acc[f] += cf * row[f]; mag[f] += std::fabs(cf * row[f]); }
                }
            }
            for (size_t f = 0; f < F; f++) {
                if (ext) {
                    const double want = pos[f] < 0 ? 0.0 : sign * acc[f];
                    if ((double)r.out[i * F + f] != want || (long long)r.arg[i * F + f] != pos[f]) {
                        if (errors++ < 10) std::cout << "error at row " << i << " column " << f << ": " << r.out[i * F + f] << " at " << r.arg[i * F + f] << " vs " << want << " at " << pos[f] << std::endl;
                    }
                } else {
                    const double scale = mean && len > 0 ? (double)len : 1.0;
                    judge("out", i * F + f, r.out[i * F + f], acc[f] / scale, mag[f] / scale, len);
                }
            }
        }
        if (o.backward) {
            // gx[u] = the sum over the entries with adj[p] = u in ascending p: the rows in order, the entries of a row in order
            std::vector<double> gacc(V * F, 0.0), gmag(V * F, 0.0);
            std::vector<long long> deg(V, 0);
            for (size_t i = 0; i < V; i++)
                for (long long p = h.rowptr[i]; p < h.rowptr[i + 1]; p++) {
                    const size_t u = (size_t)h.adj[(size_t)p];
                    deg[u]++;
                    double cf = o.weighted ? (double)w[(size_t)p] : 1.0;
                    if (mean) cf = cf / (double)(h.rowptr[i + 1] - h.rowptr[i]);
                    for (size_t f = 0; f < F; f++) {
                        const double t = (ext ? ((long long)r.arg[i * F + f] == p ? 1.0 : 0.0) : cf) * g[i * F + f];
                        gacc[u * F + f] += t; gmag[u * F + f] += std::fabs(t);
                    }
                }
            for (size_t u = 0; u < V; u++)
                for (size_t f = 0; f < F; f++) judge("gx", u * F + f, r.gx[u * F + f], gacc[u * F + f], gmag[u * F + f], deg[u]);
        }
        host.end();
        std::cout << "host restatement: " << host.get_time() * 1000.0 << " ms" << std::endl;
        std::cout << "largest error / bound: " << worst << std::endl;
        std::cout << "error count: " << errors << std::endl;
        return errors;
    }
};
#define AGG NeighbourAggregation
