// Host side of the Reduce* family (include/rten_hip_graph.hpp): the int32 ReduceL1 / ReduceSumSquare / ReduceProd of host values that shape arithmetic of
// dynamic-axes exports keeps on the host (hostops::reduce_i32: two's complement wrapping, tests/reduce_rules.py), and what the loader refuses about
// LpNormalization and Reduce* nodes by node name -- the checks rten_hip_run --parse-only runs without a device.  Also the host-side input checks of the
// C++ operators that need no launch.  Needs no GPU.
#include <cstdio>
#include <limits>
#include <string>

#include "rten_hip_graph.hpp"

using namespace rten_hip;
static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static HostVal ints(std::vector<int64_t> shape, std::vector<int64_t> v) { return hostops::make_ints(std::move(shape), std::move(v)); }
typedef std::vector<int64_t> V;

static onnx::Attr int_attr(const char *name, int64_t v) { onnx::Attr a; a.name = name; a.type = 2; a.i = v; return a; }

template <class F> static std::string graph_error(F f) {
    try { f(); } catch (const GraphError &e) { return e.what(); }
    return "";
}
static bool has(const std::string &s, const char *part) { return s.find(part) != std::string::npos; }

int main() {
    const int64_t imin = std::numeric_limits<int32_t>::min(), imax = std::numeric_limits<int32_t>::max();
    // ---- ReduceProd(Shape(x)): the element count of a dynamic shape
    HostVal y = hostops::reduce_i32(ints({4}, {2, 3, 5, 7}), {0}, false, RTEN_HIP_REDUCE_PROD);
    CHECK(!y.is_float && y.shape.empty() && y.i == V({210}));
    y = hostops::reduce_i32(ints({4}, {2, 3, 5, 7}), {0}, true, RTEN_HIP_REDUCE_PROD);
    CHECK(y.shape == V({1}) && y.i == V({210}));
    // the reference's literals (reduce.rs test_reduce_prod / test_reduce_l1 / test_reduce_sum_square)
    CHECK(hostops::reduce_i32(ints({5}, {1, 2, 3, 4, 5}), {0}, false, RTEN_HIP_REDUCE_PROD).i == V({120}));
    CHECK(hostops::reduce_i32(ints({5}, {1, 2, 3, 4, 5}), {0}, false, RTEN_HIP_REDUCE_SUM_SQUARE).i == V({55}));
    y = hostops::reduce_i32(ints({2, 3}, {-1, 2, -3, 4, -5, 6}), {1}, false, RTEN_HIP_REDUCE_L1);
    CHECK(y.shape == V({2}) && y.i == V({6, 15}));
    // axis 0 of a matrix, and both axes; keepdims shapes
    y = hostops::reduce_i32(ints({2, 3}, {-1, 2, -3, 4, -5, 6}), {0}, true, RTEN_HIP_REDUCE_L1);
    CHECK(y.shape == V({1, 3}) && y.i == V({5, 7, 9}));
    y = hostops::reduce_i32(ints({2, 3}, {-1, 2, -3, 4, -5, 6}), {0, 1}, true, RTEN_HIP_REDUCE_PROD);
    CHECK(y.shape == V({1, 1}) && y.i == V({-720}));
    y = hostops::reduce_i32(ints({2, 3}, {-1, 2, -3, 4, -5, 6}), {0}, false, RTEN_HIP_REDUCE_SUM_SQUARE);
    CHECK(y.shape == V({3}) && y.i == V({17, 29, 45}));
    // wrapping: 65536 * 65536 = 2^32 -> 0; 46341^2 = 2147488281 -> -2147479015; |i32::MIN| = i32::MIN; i32::MAX + 1 -> i32::MIN
    CHECK(hostops::reduce_i32(ints({2}, {65536, 65536}), {0}, false, RTEN_HIP_REDUCE_PROD).i == V({0}));
    CHECK(hostops::reduce_i32(ints({1}, {46341}), {0}, false, RTEN_HIP_REDUCE_SUM_SQUARE).i == V({-2147479015}));
    CHECK(hostops::reduce_i32(ints({1}, {imin}), {0}, false, RTEN_HIP_REDUCE_L1).i == V({imin}));
    CHECK(hostops::reduce_i32(ints({2}, {imax, -1}), {0}, false, RTEN_HIP_REDUCE_L1).i == V({imin}));
    CHECK(hostops::reduce_i32(ints({3}, {imin, -1, 3}), {0}, false, RTEN_HIP_REDUCE_PROD).i == V({imin})); // (MIN * -1 = MIN) * 3 = MIN (wrapping)
    // empty slices: sums 0, Prod 1; an empty kept dim gives an empty result
    CHECK(hostops::reduce_i32(ints({0}, {}), {0}, false, RTEN_HIP_REDUCE_PROD).i == V({1}));
    CHECK(hostops::reduce_i32(ints({0}, {}), {0}, false, RTEN_HIP_REDUCE_L1).i == V({0}));
    y = hostops::reduce_i32(ints({2, 0}, {}), {1}, true, RTEN_HIP_REDUCE_SUM_SQUARE);
    CHECK(y.shape == V({2, 1}) && y.i == V({0, 0}));
    y = hostops::reduce_i32(ints({2, 0}, {}), {0}, false, RTEN_HIP_REDUCE_PROD);
    CHECK(y.shape == V({0}) && y.i.empty());

    // ---- what the loader refuses, by node name, with no device
    onnx::Node lp;
    lp.op_type = "LpNormalization";
    lp.name = "head/normalize";
    lp.inputs = {"x"};
    lp.outputs = {"y"};
    Graph::LpNormNode a = Graph::read_lp_norm_node(lp, lp.name);
    CHECK(a.axis == -1 && a.p == 2); // onnx_registry.rs:1284-1287
    lp.attrs = {int_attr("axis", 1), int_attr("p", 1)};
    a = Graph::read_lp_norm_node(lp, lp.name);
    CHECK(a.axis == 1 && a.p == 1);
    lp.attrs = {int_attr("p", 3)};
    std::string msg = graph_error([&] { Graph::read_lp_norm_node(lp, lp.name); });
    CHECK(has(msg, "LpNormalization head/normalize") && has(msg, "`p` must be 1 or 2") && has(msg, "p = 3"));
    lp.attrs = {int_attr("p", 0)};
    CHECK(has(graph_error([&] { Graph::read_lp_norm_node(lp, lp.name); }), "`p` must be 1 or 2"));

    CHECK(Graph::reduce_family_kind("ReduceL1") == RTEN_HIP_REDUCE_L1 && Graph::reduce_family_kind("ReduceSumSquare") == RTEN_HIP_REDUCE_SUM_SQUARE);
    CHECK(Graph::reduce_family_kind("ReduceL2") == RTEN_HIP_REDUCE_L2 && Graph::reduce_family_kind("ReduceLogSum") == RTEN_HIP_REDUCE_LOG_SUM);
    CHECK(Graph::reduce_family_kind("ReduceLogSumExp") == RTEN_HIP_REDUCE_LOG_SUM_EXP && Graph::reduce_family_kind("ReduceProd") == RTEN_HIP_REDUCE_PROD);
    CHECK(Graph::reduce_family_kind("ReduceSum") < 0 && Graph::reduce_family_kind("ReduceMax") < 0 && Graph::reduce_family_kind("Softmax") < 0);
    onnx::Model m;
    onnx::ValueInfo gx, gaxes;
    gx.name = "x"; gx.elem_type = onnx::FLOAT;
    gaxes.name = "axes"; gaxes.elem_type = onnx::INT64;
    m.inputs = {gx, gaxes};
    onnx::Node rd;
    rd.op_type = "ReduceL2";
    rd.name = "pool/norm";
    rd.inputs = {"x", "axes"};
    rd.outputs = {"n"};
    msg = graph_error([&] { Graph::check_reduce_node(m, rd, rd.name); });
    CHECK(has(msg, "ReduceL2 pool/norm") && has(msg, "the axes input must be a constant") && has(msg, "\"axes\""));
    onnx::TensorProto init;
    init.name = "axes"; init.dims = {1}; init.data_type = onnx::INT64;
    m.initializers = {init}; // an initializer of that name: a constant, whatever the input list says
    CHECK(graph_error([&] { Graph::check_reduce_node(m, rd, rd.name); }).empty());
    rd.inputs = {"x"};
    m.initializers.clear();
    CHECK(graph_error([&] { Graph::check_reduce_node(m, rd, rd.name); }).empty());

    // ---- registry and operator defaults
    const OpRegistry reg = OpRegistry::with_all_ops();
    for (const char *k : {"ReduceL1", "ReduceL2", "ReduceSumSquare", "ReduceLogSum", "ReduceLogSumExp", "ReduceProd", "LpNormalization", "GlobalMaxPool"}) {
        CHECK(reg.contains(k));
        CHECK(std::string(reg.create(k)->name()) == k);
    }
    CHECK(ReduceL2().keep_dims && !ReduceL2().noop_with_empty_axes && ReduceL2().axes.empty() && ReduceProd().max_inputs() == 2);
    CHECK(LpNormalization().axis == -1 && LpNormalization().p == 2 && LpNormalization().max_inputs() == 1 && GlobalMaxPool().max_inputs() == 1);
    CHECK(ReduceL1().int32 && ReduceSumSquare().int32 && ReduceProd().int32 && !ReduceL2().int32 && !ReduceLogSum().int32 && !ReduceLogSumExp().int32);

    // ---- the kept / reduced split every strided reduction hands to the ABI, on the views whose lists tests/test_reduce_ops.py and tests/test_select_ops.py
    // pin for the Python layer (test_reduce_stride_lists_of_views, test_reduce_stride_lists_of_a_permuted_view): one table for both layers
    namespace E = einsum_detail;
    typedef std::vector<V> VV;
    E::View perm; // [2, 3, 4, 5] permuted by (2, 0, 3, 1)
    perm.shape = {4, 2, 5, 3};
    perm.strides = {5, 60, 1, 20};
    E::Split s = E::split_dims(perm, {1, 3});
    CHECK(s.kshape == V({4, 5}) && s.mo == V({20}) && s.mos == VV({{1}}) && s.mi == V({6}) && s.mis == VV({{20}})); // 4 x 5 merge, and 2 x 3 (60 = 20 * 3)
    s = E::split_dims(perm, {0, 2});
    CHECK(s.kshape == V({2, 3}) && s.mo == V({6}) && s.mos == VV({{20}}) && s.mi == V({20}) && s.mis == VV({{1}})); // the mirror image
    s = E::split_dims(perm, {2});
    CHECK(s.kshape == V({4, 2, 3}) && s.mo == V({4, 6}) && s.mos == VV({{5, 20}}) && s.mi == V({5}) && s.mis == VV({{1}})); // 2 x 3 merge, 4 stays apart
    E::View sliced; // a step-2 slice of the last axis: nothing merges with it
    sliced.shape = {2, 3, 4, 3};
    sliced.strides = {60, 20, 5, 2};
    s = E::split_dims(sliced, {3});
    CHECK(s.kshape == V({2, 3, 4}) && s.mo == V({24}) && s.mos == VV({{5}}) && s.mi == V({3}) && s.mis == VV({{2}}));
    // TopK's two stride lists: along dim 2 of the permuted view, k = 2, the outputs are [4, 2, 2, 3] with strides 12, 6, 3, 1 -- kept 2 x 3 would merge
    // in the view, not in them
    s = E::split_dims(perm, {2}, {V({12, 6, 3, 1})});
    CHECK(s.mo == V({4, 2, 3}) && s.mos == VV({{5, 60, 20}, {12, 6, 1}}) && s.mi == V({5}) && s.mis == VV({{1}}));
    E::View dense; // along the last dim of the contiguous tensor every kept dim merges in both lists
    dense.shape = {2, 3, 4, 5};
    dense.strides = {60, 20, 5, 1};
    s = E::split_dims(dense, {3}, {V({24, 8, 2, 1})});
    CHECK(s.mo == V({24}) && s.mos == VV({{5}, {2}}) && s.mi == V({5}) && s.mis == VV({{1}}));
    // more than 6 levels: refused with the family's words, or left to the caller (Einsum's own wording)
    E::View wide;
    wide.shape = V(7, 2);
    wide.strides = {1000000, 100000, 10000, 1000, 100, 10, 1};
    try { E::split_dims(wide, {}); CHECK(false); } catch (const OpError &e) { CHECK(std::string(e.what()).find("more than 6 non-mergeable dims") != std::string::npos); }
    CHECK(E::split_dims(wide, {}, {}, nullptr).mo.size() == 7);
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
