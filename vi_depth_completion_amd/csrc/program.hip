// Programs: a whole network (or the whole per-frame path) recorded once as an array of launch descriptors and executed
// by ONE native call -- eagerly (one launch per op, optional fork/join across up to VIDC_MAX_STREAMS HIP streams) or as
// a captured hipGraph.  This is what replaces the reference's ~1500 Python-dispatched ATen calls per frame
// (SURVEY.md §2.2): the Python host crosses the C ABI once per frame, not once per layer.
#include "common.h"
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

struct vidc_program {
    std::vector<vidc_op> ops;
    hipStream_t side[VIDC_MAX_STREAMS] = {nullptr, nullptr, nullptr, nullptr};   // [0] unused: the caller's stream
    hipEvent_t ev[VIDC_MAX_STREAMS] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t fork_ev = nullptr;
    int n_streams = 1;
    hipGraph_t graph[VIDC_MAX_SEGMENTS] = {};      // [0] = the whole program (vidc_program_capture) or segment 0
    hipGraphExec_t exec[VIDC_MAX_SEGMENTS] = {};
    std::vector<hipEvent_t> op_ev;   // per-op timing events (eager timing mode)
};

namespace {

// ---- ops: kind -> entry point, and the slots of vidc_generic_args as a function of the entry's declaration (include/vidc.h) ----------
struct Cursor { int p = 0, i = 0, f = 0; };      // the next free slot of each class

// One parameter type: its class char, the slots it takes, and how it is read.  No primary definition: an entry with a parameter of any
// other type does not compile.
template <class T> struct Arg;
template <class T> struct Arg<T*> {
    static constexpr char cls = 'p';
    static constexpr int np = 1, ni = 0, nf = 0;
    static T* get(const vidc_generic_args& g, Cursor& n) { return static_cast<T*>(const_cast<void*>(g.p[n.p++])); }
};
template <> struct Arg<int> {
    static constexpr char cls = 'i';
    static constexpr int np = 0, ni = 1, nf = 0;
    static int get(const vidc_generic_args& g, Cursor& n) { return g.i[n.i++]; }
};
template <> struct Arg<float> {
    static constexpr char cls = 'f';
    static constexpr int np = 0, ni = 0, nf = 1;
    static float get(const vidc_generic_args& g, Cursor& n) { return g.f[n.f++]; }
};
template <> struct Arg<long long> {      // low word, then high word
    static constexpr char cls = 'l';
    static constexpr int np = 0, ni = 2, nf = 0;
    static long long get(const vidc_generic_args& g, Cursor& n) {
        const uint64_t lo = (uint32_t)g.i[n.i], hi = (uint32_t)g.i[n.i + 1];
        n.i += 2;
        return (long long)(lo | hi << 32);
    }
};

// An entry int fn(A..., vidc_stream_t): K... indexes its parameters without the stream.
template <class Seq, class... A> struct Entry;
template <size_t... K, class... A> struct Entry<std::index_sequence<K...>, A...> {
    using all = std::tuple<A...>;
    template <size_t k> using arg = Arg<std::tuple_element_t<k, all>>;
    static_assert(std::is_same_v<std::tuple_element_t<sizeof...(K), all>, vidc_stream_t>, "an entry's last parameter is the stream");
    static_assert((0 + ... + arg<K>::np) <= 8 && (0 + ... + arg<K>::ni) <= 16 && (0 + ... + arg<K>::nf) <= 8,
                  "the entry needs more slots than vidc_generic_args has");
    static constexpr char classes[] = {arg<K>::cls..., '\0'};
    template <int (*Fn)(A...)> static int call(const vidc_generic_args& g, vidc_stream_t s) {
        Cursor n;
        std::tuple<A...> args{arg<K>::get(g, n)..., s};      // a braced list: evaluated left to right, so each class's slots go in declaration order
        return std::apply(Fn, args);
    }
};
template <class... A> Entry<std::make_index_sequence<sizeof...(A) - 1>, A...> entry_of(int (*)(A...));

int program_copy(const void* src, void* dst, long long bytes, vidc_stream_t s) {
    VIDC_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, vidc::as_stream(s)));
    return VIDC_OK;
}

struct OpRow {
    int kind;
    const char* name;
    const char* classes;
    int (*call)(const vidc_generic_args&, vidc_stream_t);
};
#define VIDC_OP_ROW(kind, fn) {kind, #fn, decltype(entry_of(&fn))::classes, &decltype(entry_of(&fn))::template call<&fn>}
constexpr OpRow kOps[] = {      // row k = kind k
    {},
    VIDC_OP_ROW(VIDC_OP_CONV, vidc_conv2d_bn_act),      // (launched with op.u.conv, not through `call`)
    VIDC_OP_ROW(VIDC_OP_STEM, vidc_stem_conv3x3s2),
    VIDC_OP_ROW(VIDC_OP_MAXPOOL, vidc_maxpool3x3s2),
    VIDC_OP_ROW(VIDC_OP_UPSAMPLE, vidc_upsample_bilinear_ac),
    VIDC_OP_ROW(VIDC_OP_HEAD, vidc_head_conv1x1_upsample),
    VIDC_OP_ROW(VIDC_OP_WARP_PARAMS, vidc_warp2dof_params),
    VIDC_OP_ROW(VIDC_OP_WARP_FWD, vidc_warp2dof_fwd),
    VIDC_OP_ROW(VIDC_OP_WARP_INV, vidc_warp2dof_inv_rot_norm),
    VIDC_OP_ROW(VIDC_OP_COPY, program_copy),
    VIDC_OP_ROW(VIDC_OP_SPLIT, vidc_split_bf16x3),
    VIDC_OP_ROW(VIDC_OP_AVGPOOL, vidc_avgpool2d),
    VIDC_OP_ROW(VIDC_OP_NORMALIZE, vidc_normalize_nchw),
    VIDC_OP_ROW(VIDC_OP_DET_IM2COL, vidc_det_stem_im2col),
    VIDC_OP_ROW(VIDC_OP_NEAREST2X, vidc_upsample_nearest2x),
    {},                                                 // 15: retired
    VIDC_OP_ROW(VIDC_OP_MASK, vidc_mask_scale),
    VIDC_OP_ROW(VIDC_OP_WINO_IN, vidc_winograd_input_transform),
    VIDC_OP_ROW(VIDC_OP_WINO_OUT, vidc_winograd_output_transform),
    VIDC_OP_ROW(VIDC_OP_QUANT, vidc_quant_mxfp8),
    VIDC_OP_ROW(VIDC_OP_CAST, vidc_cast_bf16),
    VIDC_OP_ROW(VIDC_OP_STEM_WARPED, vidc_stem_conv3x3s2_warped),
};
#undef VIDC_OP_ROW
constexpr int kOpRows = (int)(sizeof(kOps) / sizeof(kOps[0]));
constexpr bool rows_in_kind_order() {
    for (int k = 0; k < kOpRows; ++k)
        if (kOps[k].name && kOps[k].kind != k) return false;
    return true;
}
static_assert(kOpRows == VIDC_OP_STEM_WARPED + 1 && rows_in_kind_order(), "kOps: row k must hold kind k");

const OpRow* op_row(int kind) { return kind > 0 && kind < kOpRows && kOps[kind].name ? &kOps[kind] : nullptr; }

int launch_op(const vidc_op& op, hipStream_t st) {
    vidc_stream_t s = reinterpret_cast<vidc_stream_t>(st);
    if (op.kind == VIDC_OP_CONV) return vidc_conv2d_bn_act(&op.u.conv, s);
    const OpRow* row = op_row(op.kind);
    if (!row) {
        vidc::set_error("program: unknown op kind %d", op.kind);
        return VIDC_ERR_SHAPE;
    }
    return row->call(op.u.g, s);
}

// Issues every op; ops with stream_id k>0 go to the program's side stream k.  Dependencies across stream ids are
// expressed by wait_mask (join on everything issued so far on those ids).  Works identically under stream capture,
// where the event record/wait pairs become graph edges.
int issue(vidc_program* p, hipStream_t main, bool timing, size_t begin = 0, size_t end = (size_t)-1) {
    if (end > p->ops.size()) end = p->ops.size();
    hipStream_t st[VIDC_MAX_STREAMS];
    st[0] = main;
    for (int k = 1; k < VIDC_MAX_STREAMS; ++k) st[k] = p->side[k];
    bool forked[VIDC_MAX_STREAMS] = {true, false, false, false};
    bool dirty[VIDC_MAX_STREAMS] = {false, false, false, false};
    for (size_t i = begin; i < end; ++i) {
        const vidc_op& op = p->ops[i];
        const int sid = op.stream_id;
        if (!forked[sid]) {   // side stream joins the main stream's history on first use
            VIDC_HIP(hipEventRecord(p->fork_ev, main));
            VIDC_HIP(hipStreamWaitEvent(st[sid], p->fork_ev, 0));
            forked[sid] = true;
        }
        for (int k = 0; k < p->n_streams; ++k)
            if (k != sid && (op.wait_mask >> k & 1)) {
                VIDC_HIP(hipEventRecord(p->ev[k], st[k]));
                VIDC_HIP(hipStreamWaitEvent(st[sid], p->ev[k], 0));
                if (sid == 0) dirty[k] = false;
            }
        if (timing) VIDC_HIP(hipEventRecord(p->op_ev[i], st[sid]));
        int rc = launch_op(op, st[sid]);
        if (rc != VIDC_OK) return rc;
        dirty[sid] = true;
    }
    if (timing) VIDC_HIP(hipEventRecord(p->op_ev[end], main));
    for (int k = 1; k < p->n_streams; ++k)   // final join: the caller's stream owns everything afterwards
        if (forked[k] && dirty[k]) {
            VIDC_HIP(hipEventRecord(p->ev[k], st[k]));
            VIDC_HIP(hipStreamWaitEvent(main, p->ev[k], 0));
        }
    return VIDC_OK;
}

}  // namespace

extern "C" int vidc_op_info(int kind, vidc_op_entry* out) {
    VIDC_REQUIRE(out, VIDC_ERR_NULL, "vidc_op_info: null pointer");
    const OpRow* row = op_row(kind);
    VIDC_REQUIRE(row, VIDC_ERR_SHAPE, "vidc_op_info: unknown op kind %d", kind);
    out->name = row->name;
    out->classes = row->classes;
    return VIDC_OK;
}

extern "C" int vidc_program_create(const vidc_op* ops, int n_ops, vidc_program** out) {
    VIDC_REQUIRE(ops && out, VIDC_ERR_NULL, "vidc_program_create: null pointer");
    VIDC_REQUIRE(n_ops > 0, VIDC_ERR_SHAPE, "vidc_program_create: empty program");
    vidc_program* p = new vidc_program();
    p->ops.assign(ops, ops + n_ops);
    for (const vidc_op& op : p->ops) {
        if (op.stream_id < 0 || op.stream_id >= VIDC_MAX_STREAMS) {
            delete p;
            vidc::set_error("vidc_program_create: stream_id %d out of range", op.stream_id);
            return VIDC_ERR_SHAPE;
        }
        if (op.stream_id + 1 > p->n_streams) p->n_streams = op.stream_id + 1;
    }
    hipError_t e = hipSuccess;
    for (int k = 1; k < p->n_streams && e == hipSuccess; ++k) e = hipStreamCreateWithFlags(&p->side[k], hipStreamNonBlocking);
    for (int k = 0; k < p->n_streams && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&p->ev[k], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->fork_ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        vidc::set_error("vidc_program_create: stream/event creation failed: %s", hipGetErrorString(e));
        vidc_program_destroy(p);      // frees whatever was created
        return VIDC_ERR_HIP;
    }
    *out = p;
    return VIDC_OK;
}

extern "C" int vidc_program_run(vidc_program* p, vidc_stream_t stream) {
    VIDC_REQUIRE(p, VIDC_ERR_STATE, "vidc_program_run: null program");
    return issue(p, vidc::as_stream(stream), false);
}

namespace {
int capture_range(vidc_program* p, hipStream_t st, size_t begin, size_t end, int seg) {
    if (p->exec[seg]) { hipGraphExecDestroy(p->exec[seg]); p->exec[seg] = nullptr; }
    if (p->graph[seg]) { hipGraphDestroy(p->graph[seg]); p->graph[seg] = nullptr; }
    VIDC_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    int rc = issue(p, st, false, begin, end);
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(st, &g);
    if (rc != VIDC_OK) { if (g) hipGraphDestroy(g); return rc; }
    if (e != hipSuccess) { vidc::set_error("hipStreamEndCapture failed: %s", hipGetErrorString(e)); return VIDC_ERR_HIP; }
    p->graph[seg] = g;
    VIDC_HIP(hipGraphInstantiate(&p->exec[seg], p->graph[seg], nullptr, nullptr, 0));
    return VIDC_OK;
}
}  // namespace

extern "C" int vidc_program_capture(vidc_program* p, vidc_stream_t stream) {
    VIDC_REQUIRE(p, VIDC_ERR_STATE, "vidc_program_capture: null program");
    hipStream_t st = vidc::as_stream(stream);
    VIDC_REQUIRE(st != nullptr, VIDC_ERR_STATE, "vidc_program_capture: needs a non-default stream");
    return capture_range(p, st, 0, p->ops.size(), 0);
}

extern "C" int vidc_program_launch(vidc_program* p, vidc_stream_t stream) {
    VIDC_REQUIRE(p && p->exec[0], VIDC_ERR_STATE, "vidc_program_launch: program not captured");
    for (int k = 0; k < VIDC_MAX_SEGMENTS && p->exec[k]; ++k)      // a program captured in segments replays all of them, in order
        VIDC_HIP(hipGraphLaunch(p->exec[k], vidc::as_stream(stream)));
    return VIDC_OK;
}

// Segments: ops [begin, end) of a program as their own eager run / hipGraph, so the host can interleave other work
// (the plane block and its device->host read) between parts of one planned program.
extern "C" int vidc_program_run_range(vidc_program* p, vidc_stream_t stream, int begin, int end) {
    VIDC_REQUIRE(p, VIDC_ERR_STATE, "vidc_program_run_range: null program");
    VIDC_REQUIRE(begin >= 0 && begin < end && (size_t)end <= p->ops.size(), VIDC_ERR_SHAPE, "vidc_program_run_range: bad range [%d, %d)", begin, end);
    return issue(p, vidc::as_stream(stream), false, (size_t)begin, (size_t)end);
}

extern "C" int vidc_program_capture_range(vidc_program* p, vidc_stream_t stream, int begin, int end, int segment) {
    VIDC_REQUIRE(p, VIDC_ERR_STATE, "vidc_program_capture_range: null program");
    VIDC_REQUIRE(begin >= 0 && begin < end && (size_t)end <= p->ops.size(), VIDC_ERR_SHAPE, "vidc_program_capture_range: bad range [%d, %d)", begin, end);
    VIDC_REQUIRE(segment >= 0 && segment < VIDC_MAX_SEGMENTS, VIDC_ERR_SHAPE, "vidc_program_capture_range: segment %d out of range", segment);
    hipStream_t st = vidc::as_stream(stream);
    VIDC_REQUIRE(st != nullptr, VIDC_ERR_STATE, "vidc_program_capture_range: needs a non-default stream");
    return capture_range(p, st, (size_t)begin, (size_t)end, segment);
}

extern "C" int vidc_program_launch_segment(vidc_program* p, vidc_stream_t stream, int segment) {
    VIDC_REQUIRE(p && segment >= 0 && segment < VIDC_MAX_SEGMENTS && p->exec[segment], VIDC_ERR_STATE,
                 "vidc_program_launch_segment: segment not captured");
    VIDC_HIP(hipGraphLaunch(p->exec[segment], vidc::as_stream(stream)));
    return VIDC_OK;
}

extern "C" int vidc_program_time(vidc_program* p, vidc_stream_t stream, int iters, int use_graph, float* ms_out, float* per_op_ms) {
    VIDC_REQUIRE(p && ms_out, VIDC_ERR_NULL, "vidc_program_time: null pointer");
    VIDC_REQUIRE(iters > 0, VIDC_ERR_SHAPE, "vidc_program_time: iters must be > 0");
    hipStream_t st = vidc::as_stream(stream);
    hipEvent_t t0, t1;
    VIDC_HIP(hipEventCreate(&t0));
    VIDC_HIP(hipEventCreate(&t1));
    int rc = VIDC_OK;
    if (per_op_ms && !use_graph) {
        const size_t n = p->ops.size();
        if (p->op_ev.size() != n + 1) {
            p->op_ev.resize(n + 1);
            for (auto& e : p->op_ev) VIDC_HIP(hipEventCreate(&e));
        }
        for (size_t i = 0; i < n; ++i) per_op_ms[i] = 0.f;
        float total = 0.f;
        for (int it = 0; it < iters && rc == VIDC_OK; ++it) {
            rc = issue(p, st, true);
            if (rc != VIDC_OK) break;
            VIDC_HIP(hipStreamSynchronize(st));
            for (size_t i = 0; i < n; ++i) {   // start-to-next-start on the issuing order (exact when single-stream)
                float ms = 0.f;
                hipEventElapsedTime(&ms, p->op_ev[i], p->op_ev[i + 1]);
                per_op_ms[i] += ms / iters;
            }
            float ms = 0.f;
            hipEventElapsedTime(&ms, p->op_ev[0], p->op_ev[n]);
            total += ms;
        }
        ms_out[0] = total / iters;
    } else {
        VIDC_HIP(hipEventRecord(t0, st));
        for (int it = 0; it < iters && rc == VIDC_OK; ++it)
            rc = use_graph ? vidc_program_launch(p, stream) : issue(p, st, false);
        VIDC_HIP(hipEventRecord(t1, st));
        VIDC_HIP(hipEventSynchronize(t1));
        float ms = 0.f;
        VIDC_HIP(hipEventElapsedTime(&ms, t0, t1));
        ms_out[0] = ms / iters;
    }
    hipEventDestroy(t0);
    hipEventDestroy(t1);
    return rc;
}

extern "C" int vidc_program_destroy(vidc_program* p) {
    if (!p) return VIDC_OK;
    for (int k = 0; k < VIDC_MAX_SEGMENTS; ++k) {
        if (p->exec[k]) hipGraphExecDestroy(p->exec[k]);
        if (p->graph[k]) hipGraphDestroy(p->graph[k]);
    }
    for (int k = 1; k < VIDC_MAX_STREAMS; ++k) if (p->side[k]) hipStreamDestroy(p->side[k]);
    for (int k = 0; k < VIDC_MAX_STREAMS; ++k) if (p->ev[k]) hipEventDestroy(p->ev[k]);
    if (p->fork_ev) hipEventDestroy(p->fork_ev);
    for (auto& e : p->op_ev) hipEventDestroy(e);
    delete p;
    return VIDC_OK;
}
