// Edge scores, edge softmax and graph attention (`attn`): the fused HIP path (vgl_hip_agg_sddmm, _edge_softmax, _edge_softmax_backward and the two
// aggregation runs; the contract of include/vgl_hip.h) over a stored direction of the graph, stage by stage, and a sequential host restatement of
// each stage in float64 for -check.  The reference has no counterpart.
//   dot        e = q . k per entry;                        backward: gq = sum_p s_p k[adj p] (forward run), gk (transposed run), s a given entry gradient
//   softmax    w = softmax over each row of s;             backward: ge = w (t - sum w t), t a given entry gradient
//   attention  e = q . k, w = softmax(e), out = sum w v;   backward of out's gradient g: gw = g . v, gv, ge, gq, gk
// q holds the scale F^-1/2 already (the C interface has no scaling call; in Python it is a torch product).
// With -heads H every stage runs its heads form (the vgl_hip_agg_*_heads calls): head h owns the columns [h D, (h + 1) D), D = F / H, the entry
// scalars are E x H, q holds D^-1/2, and the restatement runs per head with D in place of F in the bound of the dot.
// With -score add the score is the additive one of GAT (vgl_hip_agg_edge_add_heads): e = leaky_relu(a[row] + b[adj], slope) from two V x H terms
// a, b; its gradients are the two entry sums (vgl_hip_agg_edge_sum_heads, the score as the gate).  The restatement holds the score to equality of
// bits and the sums to gamma_d of the sum of |c|.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

struct GraphAttention {
    enum { DOT = 0, SOFTMAX = 1, ATTENTION = 2 };
    struct Options {
        int features = 64, stage = ATTENTION, heads = 1;
        bool outgoing = false, backward = false, use_heads = false;    // use_heads: -heads was given, the heads calls run (also with H = 1)
        bool score_add = false;                                        // -score add: the additive score in place of the dot product
        float slope = 0.2f;
        size_t H() const { return use_heads ? (size_t)heads : 1; }
    };
    // the largest error of the device expf in ulps, measured (tests/studies/expf_ulps.hip), plus one
    static constexpr double EXP_ULPS = 1.857;

    // q, k, v, g (V x F) in [-0.5, 0.5) (q times F^-1/2) and s, t (one per entry) in [-8, 8): the counter hash of the position that agg_hip uses,
    // brought from its range [0, 100) on the host; the host keeps its copies for -check
    struct Inputs {
        void *q = nullptr, *k = nullptr, *v = nullptr, *g = nullptr, *s = nullptr, *t = nullptr, *a = nullptr, *b = nullptr;
        std::vector<float> hq, hk, hv, hg, hs, ht, ha, hb;            // a, b: the V x H terms of the additive score, in [-2, 2)
        size_t V = 0, E = 0, F = 0, H = 1;
        void make(void **d, std::vector<float> &h, size_t n, unsigned long long seed, float scale)
        {
            vgl_hip_ctx *c = VGL_RUNTIME::ctx();
            VGL_HIP_CALL(vgl_hip_malloc(c, sizeof(float) * std::max<size_t>(n, 1), d));
            h.resize(n);
            if (n == 0) return;
            VGL_HIP_CALL(vgl_hip_gen_weights(c, 0, (int64_t)n, seed, (float *)*d));
            VGL_HIP_CALL(vgl_hip_memcpy_d2h(c, h.data(), *d, sizeof(float) * n));
            for (float &x : h) x = (x / 100.0f - 0.5f) * scale;
            VGL_HIP_CALL(vgl_hip_memcpy_h2d(c, *d, h.data(), sizeof(float) * n));
        }
        Inputs(VGL_Graph &graph, const vgl_csr_view &view, const Options &o, unsigned long long seed) : V((size_t)graph.get_vertices_count()), E((size_t)view.edges), F((size_t)o.features), H(o.H())
        {
            make(&q, hq, V * F, seed, 1.0f / std::sqrt((float)(F / H)));
            make(&k, hk, V * F, seed + 1, 1.0f);
            make(&v, hv, V * F, seed + 2, 1.0f);
            make(&g, hg, V * F, seed + 3, 1.0f);
            make(&s, hs, E * H, seed + 4, 16.0f);
            make(&t, ht, E * H, seed + 5, 16.0f);
            if (o.score_add) {
                make(&a, ha, V * H, seed + 6, 4.0f);
                make(&b, hb, V * H, seed + 7, 4.0f);
            }
            VGL_HIP_CALL(vgl_hip_ctx_sync(VGL_RUNTIME::ctx()));
        }
        ~Inputs()
        {
            vgl_hip_ctx *c = VGL_RUNTIME::ctx();
            for (void *p : {q, k, v, g, s, t}) vgl_hip_free(c, p);
            if (a) vgl_hip_free(c, a);
            if (b) vgl_hip_free(c, b);
        }
    };
    // what a run leaves on the host
    struct Result { std::vector<float> e, w, out, gw, ge, gq, gk, gv, gs, gt; long long entries = 0; };

    struct DeviceArray {
        void *p = nullptr; size_t n = 0;
        explicit DeviceArray(size_t count) : n(count) { VGL_HIP_CALL(vgl_hip_malloc(VGL_RUNTIME::ctx(), sizeof(float) * std::max<size_t>(n, 1), &p)); }
        ~DeviceArray() { vgl_hip_free(VGL_RUNTIME::ctx(), p); }
        float *f() const { return (float *)p; }
        std::vector<float> host() const
        {
            std::vector<float> h(n);
            if (n) VGL_HIP_CALL(vgl_hip_memcpy_d2h(VGL_RUNTIME::ctx(), h.data(), p, sizeof(float) * n));
            return h;
        }
    };

    static void print_stats(const char *what, const vgl_hip_agg_stats &s, double seconds)
    {
        std::cout << "ATTN " << what << ": rows " << s.rows << ", entries " << s.entries << ", rows short / wave / wg " << s.rows_short << " / " << s.rows_wave << " / " << s.rows_wg
                  << ", chunks " << s.chunks << ", hub rows " << s.hub_rows << ", column tiles " << s.column_tiles[0] << " / " << s.column_tiles[1] << " / " << s.column_tiles[2]
                  << ", vec " << s.vec << ", transposed " << s.transposed << (s.heads > 0 ? ", heads " + std::to_string(s.heads) : std::string()) << ", " << s.algorithmic_bytes << " bytes of the model, " << seconds * 1000.0 << " ms, "
                  << s.algorithmic_bytes / (seconds * 1e9) << " GB/s" << std::endl;
    }

    // plan (timed); every call of the stage once to heat and once timed, the transposed runs a third time (their first builds the transpose, which is
    // timed as the difference).  Returns MTEPS over the entries walked by the timed calls.
    static double hip_fused(const vgl_csr_view &view, const Inputs &in, const Options &o, Result &r, bool launches = false)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        const size_t V = in.V, E = in.E, F = in.F, H = in.H;
        const int64_t ld = (int64_t)F;
        const int32_t f = (int32_t)F, hd = (int32_t)H;
        const bool heads = o.use_heads;
        DeviceArray e(E * H), w(E * H), out(V * F), gw(E * H), ge(E * H), gq(V * F), gk(V * F), gv(V * F);
        DeviceArray gs(o.score_add ? V * H : 0), gt(o.score_add ? V * H : 0);
        vgl_hip_agg_plan *plan = nullptr;
        Timer prep;
        prep.start();
        VGL_HIP_CALL(vgl_hip_agg_plan_create(c, (const int64_t *)view.rowptr, (const int32_t *)view.adj, (int32_t)V, (int32_t)V, &plan));
        prep.end();
        if (!launches) std::cout << "ATTN plan: " << prep.get_time() * 1000.0 << " ms" << std::endl;
        double seconds = 0.0, transpose = -1.0;
        long long calls = 0;
        vgl_hip_agg_stats st;
        auto run = [&](const char *what, bool transposed, const std::function<int()> &call) {
            Timer first, tm;
            first.start();
            VGL_HIP_CALL(call());
            first.end();
            if (transposed && transpose < 0.0) VGL_HIP_CALL(call());   // the run before built the transpose: one more to heat
            tm.start();
            VGL_HIP_CALL(call());
            tm.end();
            if (transposed && transpose < 0.0) transpose = std::max(0.0, first.get_time() - tm.get_time());
            seconds += tm.get_time();
            calls++;
            if (!launches) print_stats(what, st, tm.get_time());
        };
        auto dot = [&](const float *a, const float *b, float *to) {
            return heads ? vgl_hip_agg_sddmm_heads(c, plan, a, ld, b, ld, f, hd, 0, to, &st) : vgl_hip_agg_sddmm(c, plan, a, ld, b, ld, f, 0, to, &st);
        };
        auto softmax = [&](const float *from, float *to) {
            return heads ? vgl_hip_agg_edge_softmax_heads(c, plan, from, hd, to, &st) : vgl_hip_agg_edge_softmax(c, plan, from, to, &st);
        };
        auto softmax_back = [&](const float *y, const float *gy, float *to) {
            return heads ? vgl_hip_agg_edge_softmax_backward_heads(c, plan, y, gy, hd, to, &st) : vgl_hip_agg_edge_softmax_backward(c, plan, y, gy, to, &st);
        };
        auto sum = [&](const float *weight, const float *x, float *to) {
            return heads ? vgl_hip_agg_run_heads(c, plan, VGL_HIP_AGG_SUM, weight, hd, x, ld, f, to, ld, &st)
                         : vgl_hip_agg_run(c, plan, VGL_HIP_AGG_SUM, weight, x, ld, f, to, ld, nullptr, &st);
        };
        auto sum_t = [&](const float *weight, const float *grad, float *to) {
            return heads ? vgl_hip_agg_run_transposed_heads(c, plan, VGL_HIP_AGG_SUM, weight, hd, grad, ld, f, to, ld, &st)
                         : vgl_hip_agg_run_transposed(c, plan, VGL_HIP_AGG_SUM, weight, nullptr, grad, ld, f, to, ld, &st);
        };
        // the additive score from the two V x H terms, and the sum of the gated entry gradient over the rows / over the columns
        auto add = [&](float *to) { return vgl_hip_agg_edge_add_heads(c, plan, (const float *)in.a, (int64_t)H, (const float *)in.b, (int64_t)H, hd, o.slope, to, &st); };
        auto entry_sum = [&](const float *grad, const float *gate, int transposed, float *to) {
            return vgl_hip_agg_edge_sum_heads(c, plan, grad, gate, o.slope, hd, transposed, to, (int64_t)H, &st);
        };
        const float *q = (const float *)in.q, *k = (const float *)in.k, *v = (const float *)in.v, *g = (const float *)in.g, *s = (const float *)in.s, *t = (const float *)in.t;
        if (o.score_add && o.stage != SOFTMAX) {
            run("score (add)", false, [&] { return add(e.f()); });
            if (o.stage == DOT) {
                if (o.backward) {
                    run("score backward, grad s (entry sum)", false, [&] { return entry_sum(s, e.f(), 0, gs.f()); });
                    run("score backward, grad t (transposed entry sum)", true, [&] { return entry_sum(s, e.f(), 1, gt.f()); });
                }
            } else {
                run("softmax", false, [&] { return softmax(e.f(), w.f()); });
                run("weighted sum", false, [&] { return sum(w.f(), v, out.f()); });
                if (o.backward) {
                    run("backward, grad weights (dot of g and v)", false, [&] { return dot(g, v, gw.f()); });
                    run("backward, grad v (transposed run)", true, [&] { return sum_t(w.f(), g, gv.f()); });
                    run("backward, softmax backward", false, [&] { return softmax_back(w.f(), gw.f(), ge.f()); });
                    run("backward, grad s (entry sum)", false, [&] { return entry_sum(ge.f(), e.f(), 0, gs.f()); });
                    run("backward, grad t (transposed entry sum)", true, [&] { return entry_sum(ge.f(), e.f(), 1, gt.f()); });
                }
            }
        } else if (o.stage == DOT) {
            run("dot", false, [&] { return dot(q, k, e.f()); });
            if (o.backward) {
                run("dot backward, grad q (forward run)", false, [&] { return sum(s, k, gq.f()); });
                run("dot backward, grad k (transposed run)", true, [&] { return sum_t(s, q, gk.f()); });
            }
        } else if (o.stage == SOFTMAX) {
            run("softmax", false, [&] { return softmax(s, w.f()); });
            if (o.backward) run("softmax backward", false, [&] { return softmax_back(w.f(), t, ge.f()); });
        } else {
            run("dot", false, [&] { return dot(q, k, e.f()); });
            run("softmax", false, [&] { return softmax(e.f(), w.f()); });
            run("weighted sum", false, [&] { return sum(w.f(), v, out.f()); });
            if (o.backward) {
                run("backward, grad weights (dot of g and v)", false, [&] { return dot(g, v, gw.f()); });
                run("backward, grad v (transposed run)", true, [&] { return sum_t(w.f(), g, gv.f()); });
                run("backward, softmax backward", false, [&] { return softmax_back(w.f(), gw.f(), ge.f()); });
                run("backward, grad q (forward run)", false, [&] { return sum(ge.f(), k, gq.f()); });
                run("backward, grad k (transposed run)", true, [&] { return sum_t(ge.f(), q, gk.f()); });
            }
        }
        if (!launches) {
            if (transpose >= 0.0) std::cout << "ATTN transpose: " << transpose * 1000.0 << " ms (the first transposed run less a later one)" << std::endl;
            r.e = e.host(); r.w = w.host(); r.out = out.host(); r.gw = gw.host(); r.ge = ge.host(); r.gq = gq.host(); r.gk = gk.host(); r.gv = gv.host();
            r.gs = gs.host(); r.gt = gt.host();
            r.entries = (long long)E;
        }
        VGL_HIP_CALL(vgl_hip_agg_plan_destroy(c, plan));
        if (launches) return 0.0;
        performance_stats.print_algorithm_performance_stats("ATTN (fused)", seconds, (long long)E * calls);
        return performance_stats.get_algorithm_performance(seconds, (long long)E * calls);
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
        std::cout << "ATTN launches:";
        std::vector<const char *> names{"agg_prepare", "agg_transpose", "edge_dot_short", "edge_dot_wave", "edge_dot_wg", "edge_short", "edge_wave", "edge_wg", "edge_hubs", "edge_hub_write",
                                        "agg_short", "agg_wave", "agg_wg", "agg_hubs"};
        if (o.score_add)
            for (const char *name : {"edge_add_short", "edge_add_wave", "edge_add_wg", "edge_sum_short", "edge_sum_wave", "edge_sum_wg", "edge_sum_hubs"}) names.push_back(name);
        for (const char *name : names) {
            int64_t n = 0;
            double ms = 0.0;
            VGL_HIP_CALL(vgl_hip_timing_get(c, name, &n, &ms));
            std::cout << " " << name << " " << n << " (" << ms << " ms)";
            total += n;
        }
        std::cout << ", total " << total << std::endl;
        VGL_HIP_CALL(vgl_hip_timing_enable(c, 0));
    }

    static double gamma(double k, double u) { return k * u / (1.0 - k * u); }
    // gamma_k at u = 2^-24 plus the host's own at u = 2^-53
    static double tolerance(double k) { return gamma(k, std::ldexp(1.0, -24)) + gamma(k, std::ldexp(1.0, -53)); }

    // every stage on the host in float64, entry by entry, against what the device left; the input of a stage is what the device fed it
    struct Judge {
        int errors = 0;
        double worst = 0.0;
        void operator()(const char *what, size_t at, double got, double want, double bound)
        {
            const double err = std::fabs(got - want);
            if (bound > 0.0) worst = std::max(worst, err / bound);
            if (!(err <= bound) && errors++ < 10) std::cout << "error in " << what << " at " << at << ": " << got << " vs " << want << " (bound " << bound << ")" << std::endl;
        }
    };
    // H heads: e is E x H, head hd owns the D = F / H columns from hd D on (H = 1: the single-head stage)
    static void check_dot(Judge &judge, const char *what, const HostCSR &h, size_t F, size_t H, const std::vector<float> &a, const std::vector<float> &b, const std::vector<float> &e)
    {
        const size_t D = F / H;
        for (size_t i = 0; i < (size_t)h.V; i++)
            for (long long p = h.rowptr[i]; p < h.rowptr[i + 1]; p++)
                for (size_t hd = 0; hd < H; hd++) {
                    double acc = 0.0, mag = 0.0;
                    const float *x = a.data() + i * F + hd * D, *y = b.data() + (size_t)h.adj[(size_t)p] * F + hd * D;
                    for (size_t f = 0; f < D; f++) { acc += (double)x[f] * y[f]; mag += std::fabs((double)x[f] * y[f]); }
                    judge(what, (size_t)p * H + hd, e[(size_t)p * H + hd], acc, tolerance((double)D + 2) * mag);   // D products, D - 1 additions (and the division of mean)
                }
    }
    static void check_softmax(Judge &judge, const HostCSR &h, size_t H, const std::vector<float> &e, const std::vector<float> &w)
    {
        const double u = std::ldexp(1.0, -24), eps = EXP_ULPS * std::ldexp(1.0, -23), tiny = std::ldexp(1.0, -126);
        for (size_t i = 0; i < (size_t)h.V; i++)
            for (size_t hd = 0; hd < H; hd++) {
                const long long lo = h.rowptr[i], hi = h.rowptr[i + 1];
                double m = -INFINITY, s = 0.0, R = 0.0;
                for (long long p = lo; p < hi; p++) m = std::max(m, (double)e[(size_t)p * H + hd]);
                for (long long p = lo; p < hi; p++)
                    if (e[(size_t)p * H + hd] > -INFINITY) { s += std::exp((double)e[(size_t)p * H + hd] - m); R = std::max(R, m - (double)e[(size_t)p * H + hd]); }
                // 3 (R u + eps_exp) + gamma_(d + 3), relative to the exact value, plus 2^-126
                const double rel = 3.0 * (R * u + eps) + tolerance((double)(hi - lo) + 3) + 3.0 * (R + 2.0) * std::ldexp(1.0, -53);
                for (long long p = lo; p < hi; p++) {
                    const double want = e[(size_t)p * H + hd] > -INFINITY ? std::exp((double)e[(size_t)p * H + hd] - m) / s : 0.0;
                    judge("softmax", (size_t)p * H + hd, w[(size_t)p * H + hd], want, rel * want + tiny);
                }
            }
    }
    static void check_softmax_backward(Judge &judge, const HostCSR &h, size_t H, const std::vector<float> &y, const std::vector<float> &gy, const std::vector<float> &ge)
    {
        for (size_t i = 0; i < (size_t)h.V; i++)
            for (size_t hd = 0; hd < H; hd++) {
                const long long lo = h.rowptr[i], hi = h.rowptr[i + 1];
                double d = 0.0, mag = 0.0;
                for (long long p = lo; p < hi; p++) {
                    const size_t at = (size_t)p * H + hd;
                    d += (double)y[at] * gy[at]; mag += std::fabs((double)y[at] * gy[at]);
                }
                for (long long p = lo; p < hi; p++) {
                    const size_t at = (size_t)p * H + hd;
                    judge("softmax backward", at, ge[at], (double)y[at] * ((double)gy[at] - d), tolerance((double)(hi - lo) + 3) * std::fabs((double)y[at]) * (std::fabs((double)gy[at]) + mag));
                }
            }
    }
    // out[i] = sum_p weight_p x[adj p] (forward) or out[adj p] += weight_p x[i] (transposed), within gamma_(d + 2) of the sum of magnitudes
    // (weight is E x H: column f / D weighs column f)
    static void check_sum(Judge &judge, const char *what, const HostCSR &h, size_t F, size_t H, bool transposed, const std::vector<float> &weight, const std::vector<float> &x,
                          const std::vector<float> &out)
    {
        const size_t V = (size_t)h.V, D = F / H;
        std::vector<double> acc(V * F, 0.0), mag(V * F, 0.0);
        std::vector<long long> terms(V, 0);
        for (size_t i = 0; i < V; i++)
            for (long long p = h.rowptr[i]; p < h.rowptr[i + 1]; p++) {
                const size_t u = (size_t)h.adj[(size_t)p], to = transposed ? u : i, from = transposed ? i : u;
                terms[to]++;
                for (size_t f = 0; f < F; f++) {
                    const double t = (double)weight[(size_t)p * H + f / D] * x[from * F + f];
                    acc[to * F + f] += t; mag[to * F + f] += std::fabs(t);
                }
            }
        for (size_t i = 0; i < V; i++)
            for (size_t f = 0; f < F; f++) judge(what, i * F + f, out[i * F + f], acc[i * F + f], tolerance((double)terms[i] + 2) * mag[i * F + f]);
    }

    // the additive score restated in float32: one addition, one product; equality of bits
    static void check_score(Judge &judge, const HostCSR &h, size_t H, float slope, const std::vector<float> &a, const std::vector<float> &b, const std::vector<float> &e)
    {
        for (size_t i = 0; i < (size_t)h.V; i++)
            for (long long p = h.rowptr[i]; p < h.rowptr[i + 1]; p++)
                for (size_t hd = 0; hd < H; hd++) {
                    const volatile float z = a[i * H + hd] + b[(size_t)h.adj[(size_t)p] * H + hd];
                    const volatile float want = z > 0.0f ? z : slope * z;
                    const float got = e[(size_t)p * H + hd], w = want;
                    uint32_t gb, wb;
                    memcpy(&gb, &got, 4); memcpy(&wb, &w, 4);
                    judge("score (add)", (size_t)p * H + hd, gb == wb ? 0.0 : 1.0, 0.0, 0.0);
                }
    }
    // out[i] = the sum over row i of c_p (forward) or out[adj p] += c_p (transposed), c = w or slope * w where the gate is not above 0, within
    // gamma_d of the sum of |c|, d the terms of the value
    static void check_entry_sum(Judge &judge, const char *what, const HostCSR &h, size_t H, bool transposed, float slope, const std::vector<float> &w, const std::vector<float> &gate,
                                const std::vector<float> &out)
    {
        const size_t V = (size_t)h.V;
        std::vector<double> acc(V * H, 0.0), mag(V * H, 0.0);
        std::vector<long long> terms(V, 0);
        for (size_t i = 0; i < V; i++)
            for (long long p = h.rowptr[i]; p < h.rowptr[i + 1]; p++) {
                const size_t to = transposed ? (size_t)h.adj[(size_t)p] : i;
                terms[to]++;
                for (size_t hd = 0; hd < H; hd++) {
                    const size_t at = (size_t)p * H + hd;
                    const double c = gate[at] > 0.0f ? (double)w[at] : (double)slope * w[at];
                    acc[to * H + hd] += c; mag[to * H + hd] += std::fabs(c);
                }
            }
        for (size_t i = 0; i < V; i++)
            for (size_t hd = 0; hd < H; hd++) judge(what, i * H + hd, out[i * H + hd], acc[i * H + hd], tolerance((double)terms[i]) * mag[i * H + hd]);
    }

    static int verify(const HostCSR &h, const Inputs &in, const Options &o, const Result &r)
    {
        Judge judge;
        Timer host;
        host.start();
        const size_t F = in.F, H = in.H;
        if (o.score_add && o.stage != SOFTMAX) {
            check_score(judge, h, H, o.slope, in.ha, in.hb, r.e);
            if (o.stage == DOT) {
                if (o.backward) {
                    check_entry_sum(judge, "grad s", h, H, false, o.slope, in.hs, r.e, r.gs);
                    check_entry_sum(judge, "grad t", h, H, true, o.slope, in.hs, r.e, r.gt);
                }
            } else {
                check_softmax(judge, h, H, r.e, r.w);
                check_sum(judge, "out", h, F, H, false, r.w, in.hv, r.out);
                if (o.backward) {
                    check_dot(judge, "grad weights", h, F, H, in.hg, in.hv, r.gw);
                    check_sum(judge, "grad v", h, F, H, true, r.w, in.hg, r.gv);
                    check_softmax_backward(judge, h, H, r.w, r.gw, r.ge);
                    check_entry_sum(judge, "grad s", h, H, false, o.slope, r.ge, r.e, r.gs);
                    check_entry_sum(judge, "grad t", h, H, true, o.slope, r.ge, r.e, r.gt);
                }
            }
        } else if (o.stage == DOT) {
            check_dot(judge, "dot", h, F, H, in.hq, in.hk, r.e);
            if (o.backward) {
                check_sum(judge, "grad q", h, F, H, false, in.hs, in.hk, r.gq);
                check_sum(judge, "grad k", h, F, H, true, in.hs, in.hq, r.gk);
            }
        } else if (o.stage == SOFTMAX) {
            check_softmax(judge, h, H, in.hs, r.w);
            if (o.backward) check_softmax_backward(judge, h, H, r.w, in.ht, r.ge);
        } else {
            check_dot(judge, "dot", h, F, H, in.hq, in.hk, r.e);
            check_softmax(judge, h, H, r.e, r.w);
            check_sum(judge, "out", h, F, H, false, r.w, in.hv, r.out);
            if (o.backward) {
                check_dot(judge, "grad weights", h, F, H, in.hg, in.hv, r.gw);
                check_sum(judge, "grad v", h, F, H, true, r.w, in.hg, r.gv);
                check_softmax_backward(judge, h, H, r.w, r.gw, r.ge);
                check_sum(judge, "grad q", h, F, H, false, r.ge, in.hk, r.gq);
                check_sum(judge, "grad k", h, F, H, true, r.ge, in.hq, r.gk);
            }
        }
        host.end();
        std::cout << "host restatement: " << host.get_time() * 1000.0 << " ms" << std::endl;
        std::cout << "largest error / bound: " << judge.worst << std::endl;
        std::cout << "error count: " << judge.errors << std::endl;
        return judge.errors;
    }
};
#define ATTN GraphAttention
