// Host side of GridSample and DepthToSpace in the C++ layers (include/rten_hip_ops.hpp, include/rten_hip_graph.hpp): registry membership, operator
// defaults, what the loader reads from and refuses about the two nodes by node name -- the checks rten_hip_run --parse-only runs without a device
// (onnx_registry.rs:1094-1107,1203-1212) -- and the input checks of GridSample::run / DepthToSpace::run, which refuse before anything touches the device
// (the reference's errors of test_grid_sample_invalid / test_depth_to_space; rank and type as the other 4-D float32 operators).  Needs no GPU.
#include <cstdio>
#include <string>

#include "rten_hip_graph.hpp"

using namespace rten_hip;
static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static onnx::Attr int_attr(const char *name, int64_t v) { onnx::Attr a; a.name = name; a.type = 2; a.i = v; return a; }
static onnx::Attr str_attr(const char *name, const char *v) { onnx::Attr a; a.name = name; a.type = 3; a.s = v; return a; }

// what an operator's run() refuses: "Kind(\"message\")", or "" when it did not throw
template <class F> static std::string op_error(F f) {
    try { f(); } catch (const OpError &e) { return e.what(); }
    return "";
}
// a shaped tensor with no storage: enough for the checks that come before any launch
static Tensor shaped(std::vector<int64_t> shape, DType dt = DType::F32) { return Tensor::view_at(Tensor(), 0, std::move(shape), dt); }

template <class F> static std::string graph_error(F f) {
    try { f(); } catch (const GraphError &e) { return e.what(); }
    return "";
}
static bool has(const std::string &s, const char *part) { return s.find(part) != std::string::npos; }

int main() {
    // ---- GridSample: attribute defaults and refusals
    onnx::Node gs;
    gs.op_type = "GridSample";
    gs.name = "flow/warp";
    gs.inputs = {"x", "grid"};
    gs.outputs = {"y"};
    CHECK(!Graph::read_grid_sample_node(gs, gs.name).align_corners); // onnx_registry.rs:1204: defaults to false
    gs.attrs = {int_attr("align_corners", 1), str_attr("mode", "bilinear"), str_attr("padding_mode", "zeros")};
    CHECK(Graph::read_grid_sample_node(gs, gs.name).align_corners);
    gs.attrs = {str_attr("mode", "linear")}; // the opset 20 name
    CHECK(!Graph::read_grid_sample_node(gs, gs.name).align_corners);
    for (const char *mode : {"nearest", "bicubic", "cubic", ""}) {
        gs.attrs = {str_attr("mode", mode)};
        const std::string msg = graph_error([&] { Graph::read_grid_sample_node(gs, gs.name); });
        CHECK(has(msg, "GridSample flow/warp") && has(msg, (std::string("mode=\"") + mode + "\"").c_str()));
    }
    for (const char *pad : {"border", "reflection"}) {
        gs.attrs = {str_attr("mode", "bilinear"), str_attr("padding_mode", pad)};
        const std::string msg = graph_error([&] { Graph::read_grid_sample_node(gs, gs.name); });
        CHECK(has(msg, "GridSample flow/warp") && has(msg, (std::string("padding_mode=\"") + pad + "\"").c_str()));
    }

    // ---- DepthToSpace: mode defaults to DCR, blocksize is required and must fit a u32
    onnx::Node ds;
    ds.op_type = "DepthToSpace";
    ds.name = "head/shuffle";
    ds.inputs = {"x"};
    ds.outputs = {"y"};
    ds.attrs = {int_attr("blocksize", 3)};
    Graph::DepthToSpaceNode a = Graph::read_depth_to_space_node(ds, ds.name);
    CHECK(a.block_size == 3 && a.mode == DepthToSpaceMode::DepthColumnRow);
    ds.attrs = {int_attr("blocksize", 2), str_attr("mode", "CRD")};
    a = Graph::read_depth_to_space_node(ds, ds.name);
    CHECK(a.block_size == 2 && a.mode == DepthToSpaceMode::ColumnRowDepth);
    ds.attrs = {int_attr("blocksize", 2), str_attr("mode", "DCR")};
    CHECK(Graph::read_depth_to_space_node(ds, ds.name).mode == DepthToSpaceMode::DepthColumnRow);
    ds.attrs = {int_attr("blocksize", 0)}; // read; the operator refuses it
    CHECK(Graph::read_depth_to_space_node(ds, ds.name).block_size == 0);
    ds.attrs = {int_attr("blocksize", 2), str_attr("mode", "XYZ")};
    std::string msg = graph_error([&] { Graph::read_depth_to_space_node(ds, ds.name); });
    CHECK(has(msg, "DepthToSpace head/shuffle") && has(msg, "mode=\"XYZ\""));
    ds.attrs = {str_attr("mode", "CRD")};
    msg = graph_error([&] { Graph::read_depth_to_space_node(ds, ds.name); });
    CHECK(has(msg, "DepthToSpace head/shuffle") && has(msg, "blocksize attribute is missing"));
    for (int64_t bad : {(int64_t)-1, (int64_t)1 << 32}) {
        ds.attrs = {int_attr("blocksize", bad)};
        msg = graph_error([&] { Graph::read_depth_to_space_node(ds, ds.name); });
        CHECK(has(msg, "DepthToSpace head/shuffle") && has(msg, "out of range"));
    }

    // ---- registry and operator defaults
    const OpRegistry reg = OpRegistry::with_all_ops();
    for (const char *k : {"GridSample", "DepthToSpace"}) {
        CHECK(reg.contains(k));
        CHECK(std::string(reg.create(k)->name()) == k);
    }
    CHECK(!GridSample().align_corners && GridSample().max_inputs() == 2);
    CHECK(DepthToSpace().block_size == 0 && DepthToSpace().mode == DepthToSpaceMode::DepthColumnRow && DepthToSpace().max_inputs() == 1);

    // ---- the operators' own input checks.  They throw before the context is used: a borrowed handle that is never dereferenced stands in for a device.
    {
        alignas(16) static char no_device[64];
        Context ctx(reinterpret_cast<rten_hip_ctx *>(no_device), Context::Borrow{});
        auto grid_sample = [&](const Tensor &x, const Tensor &g) { const InputList in{&x, &g}; return op_error([&] { GridSample().run(ctx, in); }); };
        CHECK(grid_sample(shaped({1, 1, 1, 1}), shaped({2, 1, 1, 2})) == "IncompatibleInputShapes(\"Batch size of input and grid must match\")");
        CHECK(grid_sample(shaped({1, 1, 1, 1}), shaped({1, 1, 1, 3})) == "UnsupportedValue(\"Unsupported grid coordinate size\")");
        CHECK(grid_sample(shaped({3, 5, 7}), shaped({1, 4, 6, 2})) == "InvalidValue(\"input must have 4 dims (NCHW)\")");
        CHECK(has(grid_sample(shaped({1, 3, 5, 7}), shaped({4, 6, 2})), "InvalidValue"));
        CHECK(has(grid_sample(shaped({1, 3, 5, 7}, DType::I32), shaped({1, 4, 6, 2})), "InputCastFailed"));
        CHECK(has(grid_sample(shaped({1, 3, 5, 7}), shaped({1, 4, 6, 2}, DType::I32)), "InputCastFailed"));
        const Tensor only = shaped({1, 3, 5, 7});
        CHECK(op_error([&] { GridSample().run(ctx, InputList{&only}); }) == "MissingInputs");
        auto depth_to_space = [&](const Tensor &x, int64_t block, DepthToSpaceMode mode) {
            DepthToSpace op;
            op.block_size = block;
            op.mode = mode;
            const InputList in{&x};
            return op_error([&] { op.run(ctx, in); });
        };
        const DepthToSpaceMode crd = DepthToSpaceMode::ColumnRowDepth, dcr = DepthToSpaceMode::DepthColumnRow;
        CHECK(depth_to_space(shaped({1, 16, 2, 2}), 3, crd) == "InvalidValue(\"input channels must be a multiple of `block_size` squared\")");
        CHECK(depth_to_space(shaped({1, 16, 2, 2}), 0, crd) == "InvalidValue(\"`block_size` must be > 0\")");
        CHECK(depth_to_space(shaped({1, 16, 2, 2}), -2, dcr) == "InvalidValue(\"`block_size` must be > 0\")");
        CHECK(depth_to_space(shaped({1, 16, 2, 2}), (int64_t)1 << 32, dcr) == "InvalidValue(\"input channels must be a multiple of `block_size` squared\")");
        CHECK(depth_to_space(shaped({16, 2, 2}), 2, dcr) == "InvalidValue(\"input must have 4 dims (NCHW)\")");
        CHECK(has(depth_to_space(shaped({1, 16, 2, 2}, DType::I32), 2, dcr), "InputCastFailed"));
        CHECK(op_error([&] { DepthToSpace().run(ctx, InputList{}); }) == "MissingInputs");
    }
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
