// Host side of CumSum, GatherElements, Trilu and Tile in the C++ layers (include/rten_hip_ops.hpp, include/rten_hip_graph.hpp): registry membership, operator and
// attribute defaults, the hostops:: functions the executor evaluates host values with against the reference's literal cases (tests/golden/index_reference.json
// restated here) and the kernels' edge rules (+0.0 + -0.0, wrapping int32, delta in 64 bits), what the loader reads from and refuses about the four nodes by
// node name -- the checks rten_hip_run --parse-only runs without a device -- and the operators' own input checks, which refuse before anything touches the
// device.  Needs no GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "rten_hip_graph.hpp"

using namespace rten_hip;
static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static onnx::Attr int_attr(const char *name, int64_t v) { onnx::Attr a; a.name = name; a.type = 2; a.i = v; return a; }
template <class F> static std::string op_error(F f) {
    try { f(); } catch (const OpError &e) { return e.what(); }
    return "";
}
template <class F> static std::string graph_error(F f) {
    try { f(); } catch (const GraphError &e) { return e.what(); }
    return "";
}
static bool has(const std::string &s, const char *part) { return s.find(part) != std::string::npos; }
static Tensor shaped(std::vector<int64_t> shape, DType dt = DType::F32) { return Tensor::view_at(Tensor(), 0, std::move(shape), dt); }
static HostVal ints(std::vector<int64_t> shape, std::vector<int64_t> v) { return hostops::make_ints(std::move(shape), std::move(v)); }
static HostVal floats(std::vector<int64_t> shape, std::vector<float> v) { HostVal h; h.shape = std::move(shape); h.is_float = true; h.f = std::move(v); return h; }
static bool same_floats(const HostVal &h, const std::vector<float> &want) { return h.is_float && h.f.size() == want.size() && std::memcmp(h.f.data(), want.data(), 4 * want.size()) == 0; }

int main() {
    // ---- hostops::cumsum: test_cum_sum's literals
    const std::vector<float> six = {0, 1, 2, 3, 4, 5};
    CHECK(same_floats(hostops::cumsum(floats({6}, six), 0, false, false), {0, 1, 3, 6, 10, 15}));
    CHECK(same_floats(hostops::cumsum(floats({6}, six), 0, true, false), {0, 0, 1, 3, 6, 10}));
    CHECK(same_floats(hostops::cumsum(floats({6}, six), 0, false, true), {15, 15, 14, 12, 9, 5}));
    CHECK(same_floats(hostops::cumsum(floats({6}, six), 0, true, true), {15, 14, 12, 9, 5, 0}));
    CHECK(same_floats(hostops::cumsum(floats({1, 4, 4}, std::vector<float>(16, 1.f)), 1, false, false), {1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4}));
    CHECK(same_floats(hostops::cumsum(floats({1, 4, 4}, std::vector<float>(16, 1.f)), -1, false, false), {1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4}));
    for (bool ex : {false, true}) for (bool rev : {false, true}) CHECK(hostops::cumsum(floats({0}, {}), 0, ex, rev).f.empty());
    CHECK(same_floats(hostops::cumsum(floats({2}, {-0.f, -0.f}), 0, false, false), {0.f, 0.f})); // +0.0 + -0.0: the sign bit is clear
    CHECK(hostops::cumsum(ints({3}, {2147483647, 1, 5}), 0, false, false).i == (std::vector<int64_t>{2147483647, -2147483648ll, -2147483643ll})); // wraps
    CHECK(hostops::cumsum(ints({2, 2}, {1, 2, 3, 4}), 0, false, false).i == (std::vector<int64_t>{1, 2, 4, 6}));
    CHECK(op_error([] { hostops::cumsum(ints({}, {1}), 0, false, false); }) == "InvalidValue(\"Axis is invalid\")"); // a rank-0 operand
    CHECK(op_error([] { hostops::cumsum(ints({2}, {1, 2}), 1, false, false); }) == "InvalidValue(\"Axis is invalid\")");

    // ---- hostops::trilu: test_trilu's literals, test_trilu_invalid
    const HostVal m3 = ints({3, 3}, {1, 2, 3, 4, 5, 6, 7, 8, 9});
    CHECK(hostops::trilu(m3, 0, true).i == (std::vector<int64_t>{1, 2, 3, 0, 5, 6, 0, 0, 9}));
    CHECK(hostops::trilu(m3, 1, true).i == (std::vector<int64_t>{0, 2, 3, 0, 0, 6, 0, 0, 0}));
    CHECK(hostops::trilu(m3, -1, true).i == (std::vector<int64_t>{1, 2, 3, 4, 5, 6, 0, 8, 9}));
    CHECK(hostops::trilu(m3, 0, false).i == (std::vector<int64_t>{1, 0, 0, 4, 5, 0, 7, 8, 9}));
    CHECK(hostops::trilu(m3, 1, false).i == (std::vector<int64_t>{1, 2, 0, 4, 5, 6, 7, 8, 9}));
    CHECK(hostops::trilu(m3, -1, false).i == (std::vector<int64_t>{0, 0, 0, 4, 0, 0, 7, 8, 0}));
    CHECK(hostops::trilu(ints({2, 3, 3}, {1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 8, 7, 6, 5, 4, 3, 2, 1}), 0, true).i == (std::vector<int64_t>{1, 2, 3, 0, 5, 6, 0, 0, 9, 9, 8, 7, 0, 5, 4, 0, 0, 1}));
    CHECK(hostops::trilu(ints({3, 5}, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}), 0, true).i == (std::vector<int64_t>{1, 2, 3, 4, 5, 0, 7, 8, 9, 10, 0, 0, 13, 14, 15}));
    CHECK(hostops::trilu(ints({5, 3}, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}), 0, true).i == (std::vector<int64_t>{1, 2, 3, 0, 5, 6, 0, 0, 9, 0, 0, 0, 0, 0, 0}));
    CHECK(op_error([] { hostops::trilu(ints({1}, {1}), 0, true); }) == "InvalidValue(\"Input must have >= 2 dims\")");
    CHECK(hostops::trilu(m3, 2147483647ll, false).i == m3.i && hostops::trilu(m3, -2147483648ll, true).i == m3.i); // delta in 64 bits: no wrap at the ends of i32
    CHECK(hostops::trilu(m3, 2147483647ll, true).i == std::vector<int64_t>(9, 0));
    CHECK(same_floats(hostops::trilu(floats({2, 2}, {NAN, NAN, NAN, NAN}), 5, true), {0.f, 0.f, 0.f, 0.f})); // a masked NaN becomes +0.0
    { // the exporter's causal mask: triu(full((3, 3), -inf), 1)
        const float ninf = -INFINITY;
        CHECK(same_floats(hostops::trilu(floats({3, 3}, std::vector<float>(9, ninf)), 1, true), {0, ninf, ninf, 0, 0, ninf, 0, 0, 0}));
    }

    // ---- hostops::tile: test_tile's literals, test_tile_invalid_repeats
    HostVal out;
    CHECK(hostops::tile(ints({3, 4, 5}, std::vector<int64_t>(60, 0)), {4, 0, 1}, out) && out.shape == (std::vector<int64_t>{12, 0, 5}) && out.i.empty());
    out = HostVal();
    CHECK(hostops::tile(ints({}, {5}), {}, out) && out.shape.empty() && out.i == (std::vector<int64_t>{5}));
    out = HostVal();
    CHECK(hostops::tile(ints({4}, {1, 2, 3, 4}), {3}, out) && out.i == (std::vector<int64_t>{1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4}));
    out = HostVal();
    CHECK(hostops::tile(ints({1, 1}, {3}), {3, 2}, out) && out.shape == (std::vector<int64_t>{3, 2}) && out.i == std::vector<int64_t>(6, 3));
    out = HostVal();
    CHECK(hostops::tile(ints({4}, {1, 2, 3, 4}), {1}, out) && out.i == (std::vector<int64_t>{1, 2, 3, 4}));
    out = HostVal();
    CHECK(hostops::tile(ints({2, 2}, {1, 2, 3, 4}), {1, 2}, out) && out.i == (std::vector<int64_t>{1, 2, 1, 2, 3, 4, 3, 4}));
    out = HostVal();
    CHECK(hostops::tile(ints({2, 2}, {1, 2, 3, 4}), {2, 1}, out) && out.i == (std::vector<int64_t>{1, 2, 3, 4, 1, 2, 3, 4}));
    out = HostVal();
    CHECK(hostops::tile(ints({2, 2}, {1, 2, 3, 4}), {2, 2}, out) && out.i == (std::vector<int64_t>{1, 2, 1, 2, 3, 4, 3, 4, 1, 2, 1, 2, 3, 4, 3, 4}));
    out = HostVal();
    CHECK(op_error([&] { hostops::tile(ints({3}, {1, 2, 3}), {1, 2}, out); }) == "InvalidValue(\"invalid repeats\")");
    CHECK(op_error([&] { hostops::tile(ints({3}, {1, 2, 3}), {-1}, out); }) == "InvalidValue(\"invalid repeats\")");
    out = HostVal();
    CHECK(!hostops::tile(ints({1}, {1}), {hostops::kMaxHostElems + 1}, out)); // too large to mirror on the host: the device runs it

    // ---- hostops::gather_elements: test_gather_elements' literals, test_gather_elements_invalid_inputs
    CHECK(hostops::gather_elements(ints({2, 2}, {1, 2, 3, 4}), ints({2, 2}, {0, 0, 1, 0}), 1).i == (std::vector<int64_t>{1, 1, 4, 3}));
    CHECK(hostops::gather_elements(m3, ints({2, 3}, {1, 2, 0, 2, 0, 0}), 0).i == (std::vector<int64_t>{4, 8, 3, 7, 2, 3}));
    CHECK(hostops::gather_elements(ints({3}, {1, 2, 3}), ints({4}, {-1, -1, -2, -2}), 0).i == (std::vector<int64_t>{3, 3, 2, 2}));
    CHECK(hostops::gather_elements(ints({1, 1, 1, 2, 2}, {1, 2, 3, 4}), ints({1, 1, 1, 2, 2}, {1, 1, 0, 0}), 4).i == (std::vector<int64_t>{2, 2, 3, 3}));
    CHECK(hostops::gather_elements(ints({0}, {}), ints({0}, {}), 0).i.empty() && hostops::gather_elements(ints({3}, {1, 2, 3}), ints({0}, {}), 0).i.empty());
    CHECK(hostops::gather_elements(ints({2, 3}, {1, 2, 3, 3, 4, 5}), ints({2, 1}, {0, 2}), 1).i == (std::vector<int64_t>{1, 5}));
    CHECK(hostops::gather_elements(m3, ints({2, 1}, {1, 2}), 0).i == (std::vector<int64_t>{4, 7}));
    CHECK(same_floats(hostops::gather_elements(floats({2, 2}, {1.5f, -0.f, 3.f, 4.f}), ints({2, 1}, {1, -2}), 1), {-0.f, 3.f}));
    const HostVal m2 = ints({2, 2}, {1, 2, 3, 4});
    CHECK(op_error([&] { hostops::gather_elements(m2, ints({2, 2}, {0, 0, 1, 0}), 2); }) == "InvalidValue(\"Axis is invalid\")");
    CHECK(op_error([&] { hostops::gather_elements(m2, ints({2, 2}, {0, 0, 1, 3}), 1); }) == "InvalidValue(\"Entry in `indices` is out of range\")");
    CHECK(op_error([&] { hostops::gather_elements(m2, ints({3}, {1, 2, 3}), 1); }) == "IncompatibleInputShapes(\"Input and indices must have same rank\")");
    CHECK(op_error([&] { hostops::gather_elements(m2, ints({2, 3}, {1, 2, 3, 4, 5, 6}), 0); }) == "IncompatibleInputShapes(\"`indices` size must be <= input size in non-axis dimensions\")");

    // ---- the loader's reads and refusals, by node name
    onnx::Model m;
    for (const char *gi : {"x", "axis_in"}) { onnx::ValueInfo v; v.name = gi; m.inputs.push_back(v); }
    { onnx::TensorProto t; t.name = "axis_c"; m.initializers.push_back(t); }
    onnx::Node n;
    n.op_type = "CumSum"; n.name = "emb/cumsum"; n.inputs = {"x", "axis_c"}; n.outputs = {"y"};
    Graph::CumSumNode c = Graph::read_cumsum_node(m, n, n.name);
    CHECK(!c.exclusive && !c.reverse); // onnx_registry.rs:1056-1060: both default to false
    n.attrs = {int_attr("exclusive", 1), int_attr("reverse", 1)};
    c = Graph::read_cumsum_node(m, n, n.name);
    CHECK(c.exclusive && c.reverse);
    n.inputs = {"x"};
    std::string msg = graph_error([&] { Graph::read_cumsum_node(m, n, n.name); });
    CHECK(has(msg, "CumSum emb/cumsum") && has(msg, "the axis input is missing"));
    n.inputs = {"x", ""};
    CHECK(has(graph_error([&] { Graph::read_cumsum_node(m, n, n.name); }), "the axis input is missing"));
    n.inputs = {"x", "axis_in"};
    msg = graph_error([&] { Graph::read_cumsum_node(m, n, n.name); });
    CHECK(has(msg, "CumSum emb/cumsum") && has(msg, "axis must be a constant or computable from the input shapes") && has(msg, "\"axis_in\""));
    n.inputs = {"x", "shape_arithmetic"}; // neither a graph input nor a constant: decided when the step runs
    Graph::read_cumsum_node(m, n, n.name);
    n.inputs = {"x", "axis_c", "x"};
    CHECK(has(graph_error([&] { Graph::read_cumsum_node(m, n, n.name); }), "takes at most 2 inputs (it has 3)"));

    n = onnx::Node();
    n.op_type = "GatherElements"; n.name = "pick"; n.inputs = {"x", "x"}; n.outputs = {"y"};
    CHECK(Graph::read_gather_elements_node(n, n.name).axis == 0); // the attribute defaults to 0
    n.attrs = {int_attr("axis", -2)};
    CHECK(Graph::read_gather_elements_node(n, n.name).axis == -2);
    n.inputs = {"x", "x", "x"};
    msg = graph_error([&] { Graph::read_gather_elements_node(n, n.name); });
    CHECK(has(msg, "GatherElements pick") && has(msg, "takes at most 2 inputs"));

    n = onnx::Node();
    n.op_type = "Trilu"; n.name = "mask"; n.inputs = {"x"}; n.outputs = {"y"};
    CHECK(Graph::read_trilu_node(m, n, n.name).upper); // defaults to upper
    n.attrs = {int_attr("upper", 0)};
    CHECK(!Graph::read_trilu_node(m, n, n.name).upper);
    n.inputs = {"x", "axis_in"};
    msg = graph_error([&] { Graph::read_trilu_node(m, n, n.name); });
    CHECK(has(msg, "Trilu mask") && has(msg, "k must be a constant or computable from the input shapes") && has(msg, "\"axis_in\""));
    n.inputs = {"x", "axis_c", "axis_c"};
    msg = graph_error([&] { Graph::read_trilu_node(m, n, n.name); });
    CHECK(has(msg, "Trilu mask") && has(msg, "takes at most 2 inputs (it has 3)"));

    n = onnx::Node();
    n.op_type = "Tile"; n.name = "rep"; n.inputs = {"x", "axis_c"}; n.outputs = {"y"};
    Graph::read_tile_node(m, n, n.name);
    n.inputs = {"x"};
    msg = graph_error([&] { Graph::read_tile_node(m, n, n.name); });
    CHECK(has(msg, "Tile rep") && has(msg, "the repeats input is missing"));
    n.inputs = {"x", "axis_in"};
    msg = graph_error([&] { Graph::read_tile_node(m, n, n.name); });
    CHECK(has(msg, "Tile rep") && has(msg, "repeats must be a constant or computable from the input shapes") && has(msg, "\"axis_in\""));
    n.inputs = {"x", "axis_c", "axis_c"};
    CHECK(has(graph_error([&] { Graph::read_tile_node(m, n, n.name); }), "takes at most 2 inputs (it has 3)"));
    for (const char *k : {"CumSum", "GatherElements", "Trilu", "Tile"}) CHECK(Graph::is_index_kind(k));
    CHECK(!Graph::is_index_kind("Gather") && !Graph::is_index_kind("ScatterElements") && !Graph::is_index_kind("GatherND"));

    // ---- registry and operator defaults
    const OpRegistry reg = OpRegistry::with_all_ops();
    for (const char *k : {"CumSum", "GatherElements", "Trilu", "Tile"}) {
        CHECK(reg.contains(k));
        CHECK(std::string(reg.create(k)->name()) == k);
        CHECK(reg.create(k)->max_inputs() == 2);
    }
    CHECK(!reg.contains("ScatterElements") && !reg.contains("GatherND") && !reg.contains("OneHot"));
    CHECK(!CumSum().exclusive && !CumSum().reverse && GatherElements().axis == 0 && Trilu().upper);

    // ---- the operators' own input checks.  They throw before the context is used: a borrowed handle that is never dereferenced stands in for a device.
    {
        alignas(16) static char no_device[64];
        Context ctx(reinterpret_cast<rten_hip_ctx *>(no_device), Context::Borrow{});
        auto host_i32 = [](std::vector<int64_t> shape, std::vector<int64_t> v) {
            Tensor t = shaped(shape, DType::I32);
            auto h = std::make_shared<HostVal>(ints(std::move(shape), std::move(v)));
            t.set_host(h);
            return t;
        };
        auto run2 = [&](const Operator &op, const Tensor &a, const Tensor &b) { const InputList in{&a, &b}; return op_error([&] { op.run(ctx, in); }); };
        CHECK(run2(CumSum(), shaped({}), host_i32({}, {0})) == "InvalidValue(\"Axis is invalid\")");
        CHECK(run2(CumSum(), shaped({2, 3}), host_i32({}, {2})) == "InvalidValue(\"Axis is invalid\")");
        CHECK(run2(CumSum(), shaped({2, 3}), host_i32({2}, {0, 1})) == "InputCastFailed(\"expected tensor with 0 dims\")");
        CHECK(has(run2(CumSum(), shaped({2, 3}), shaped({}, DType::F32)), "InputCastFailed"));
        CHECK(run2(CumSum(), shaped({2, 3}, DType::U8), host_i32({}, {0})) == "UnsupportedType");
        const Tensor only = shaped({2, 3});
        CHECK(op_error([&] { CumSum().run(ctx, InputList{&only}); }) == "MissingInputs");
        CHECK(run2(GatherElements(), shaped({2, 2}), shaped({3}, DType::I32)) == "IncompatibleInputShapes(\"Input and indices must have same rank\")");
        CHECK(run2(GatherElements(), shaped({2, 2}), shaped({2, 3}, DType::I32)) == "IncompatibleInputShapes(\"`indices` size must be <= input size in non-axis dimensions\")");
        GatherElements ge;
        ge.axis = 2;
        CHECK(run2(ge, shaped({2, 2}), shaped({2, 2}, DType::I32)) == "InvalidValue(\"Axis is invalid\")");
        ge.axis = 1;
        CHECK(run2(ge, shaped({2, 2}), host_i32({2, 2}, {0, 0, 1, 3})) == "InvalidValue(\"Entry in `indices` is out of range\")"); // host-valued indices: checked on the host
        CHECK(run2(ge, shaped({2, 2}), host_i32({2, 2}, {0, 0, 1, -3})) == "InvalidValue(\"Entry in `indices` is out of range\")");
        CHECK(run2(ge, shaped({2, 0}), shaped({2, 2}, DType::I32)) == "InvalidValue(\"Entry in `indices` is out of range\")"); // an empty axis: nothing to clamp to
        CHECK(has(run2(ge, shaped({2, 2}), shaped({2, 2})), "InputCastFailed"));
        const Tensor vec = shaped({3}, DType::I32);
        CHECK(op_error([&] { Trilu().run(ctx, InputList{&vec}); }) == "InvalidValue(\"Input must have >= 2 dims\")");
        CHECK(run2(Trilu(), shaped({2, 2}), host_i32({2}, {0, 1})) == "InputCastFailed(\"expected tensor with 0 dims\")");
        CHECK(op_error([&] { Trilu().run(ctx, InputList{}); }) == "MissingInputs");
        CHECK(run2(Tile(), vec, host_i32({2}, {1, 2})) == "InvalidValue(\"invalid repeats\")");
        CHECK(run2(Tile(), vec, host_i32({1}, {-1})) == "InvalidValue(\"invalid repeats\")");
        CHECK(run2(Tile(), shaped({2, 2}), host_i32({1, 2}, {1, 1})) == "InputCastFailed(\"expected tensor with 1 dims\")");
        CHECK(op_error([&] { Tile().run(ctx, InputList{&vec}); }) == "MissingInputs");
    }
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
