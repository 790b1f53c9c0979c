// Host side of NonMaxSuppression in the C++ layers (include/rten_hip_ops.hpp, include/rten_hip_graph.hpp): what the loader reads from and refuses about the
// node, by node name -- the checks rten_hip_run --parse-only runs without a device --, registry membership and defaults, the operator's own input checks,
// which refuse before anything touches the device, and the capture refusal, which Graph::capture decides from the plan before it runs or captures anything:
// every Context here is a borrowed handle that is never dereferenced.  Needs no GPU.
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
static Tensor host_scalar(std::vector<int64_t> shape, bool is_float, double v, size_t count = 1) {
    Tensor t = shaped(shape, is_float ? DType::F32 : DType::I32);
    auto h = std::make_shared<HostVal>();
    h->shape = std::move(shape);
    h->is_float = is_float;
    if (is_float) h->f.assign(count, (float)v); else h->i.assign(count, (int64_t)v);
    t.set_host(h);
    return t;
}

int main() {
    // ---- the loader's reads and refusals, by node name
    onnx::Model m;
    for (const char *gi : {"boxes", "scores", "cap_in", "iou_in", "score_in"}) { onnx::ValueInfo v; v.name = gi; m.inputs.push_back(v); }
    for (const char *c : {"cap_c", "iou_c", "score_c"}) { onnx::TensorProto t; t.name = c; m.initializers.push_back(t); }
    onnx::Node n;
    n.op_type = "NonMaxSuppression"; n.name = "post/nms"; n.inputs = {"boxes", "scores"}; n.outputs = {"selected"};
    Graph::NmsNode a = Graph::read_nms_node(m, n, n.name);
    CHECK(a.center_point_box == 0 && !a.has_max && !a.has_iou && !a.has_score); // center_point_box defaults to 0; every optional operand absent
    n.attrs = {int_attr("center_point_box", 1)};
    n.inputs = {"boxes", "scores", "cap_c", "iou_c", "score_c"};
    a = Graph::read_nms_node(m, n, n.name);
    CHECK(a.center_point_box == 1 && a.has_max && a.has_iou && a.has_score);
    n.inputs = {"boxes", "scores", "", "iou_c"};
    a = Graph::read_nms_node(m, n, n.name);
    CHECK(!a.has_max && a.has_iou && !a.has_score);
    n.inputs = {"boxes", "scores", "shape_arithmetic", "", "score_c"}; // neither a graph input nor a constant: decided when the step runs
    a = Graph::read_nms_node(m, n, n.name);
    CHECK(a.has_max && !a.has_iou && a.has_score);
    n.attrs = {int_attr("center_point_box", 2)};
    std::string msg = graph_error([&] { Graph::read_nms_node(m, n, n.name); });
    CHECK(has(msg, "NonMaxSuppression post/nms") && has(msg, "center_point_box 2 is not 0"));
    n.attrs = {int_attr("center_point_box", -1)};
    CHECK(has(graph_error([&] { Graph::read_nms_node(m, n, n.name); }), "center_point_box -1"));
    n.attrs.clear();
    n.inputs = {"boxes", "scores", "cap_c", "iou_c", "score_c", "cap_c"};
    msg = graph_error([&] { Graph::read_nms_node(m, n, n.name); });
    CHECK(has(msg, "NonMaxSuppression post/nms") && has(msg, "takes at most 5 inputs (it has 6)"));
    n.inputs = {"boxes"};
    CHECK(has(graph_error([&] { Graph::read_nms_node(m, n, n.name); }), "the boxes or scores input is missing"));
    const char *names[3] = {"max_output_boxes_per_class", "iou_threshold", "score_threshold"};
    const char *graph_inputs[3] = {"cap_in", "iou_in", "score_in"};
    for (int k = 0; k < 3; k++) {
        n.inputs = {"boxes", "scores", "cap_c", "iou_c", "score_c"};
        n.inputs[(size_t)(2 + k)] = graph_inputs[k];
        msg = graph_error([&] { Graph::read_nms_node(m, n, n.name); });
        CHECK(has(msg, "NonMaxSuppression post/nms") && has(msg, (std::string(names[k]) + " must be a constant or computable from the input shapes").c_str()) && has(msg, graph_inputs[k]));
    }

    // ---- registry and operator defaults
    const OpRegistry reg = OpRegistry::with_all_ops();
    CHECK(reg.contains("NonMaxSuppression") && std::string(reg.create("NonMaxSuppression")->name()) == "NonMaxSuppression" && reg.create("NonMaxSuppression")->max_inputs() == 5);
    CHECK(NonMaxSuppression().center_point_box == 0);

    alignas(16) static char no_device[64];
    Context ctx(reinterpret_cast<rten_hip_ctx *>(no_device), Context::Borrow{});
    // ---- the operator's own input checks: they throw before the context is used
    {
        auto run = [&](const Operator &op, std::vector<const Tensor *> in) { const InputList il(in.begin(), in.end()); return op_error([&] { op.run(ctx, il); }); };
        const Tensor boxes = shaped({1, 10, 4}), scores = shaped({1, 10, 10});
        const Tensor boxes3 = shaped({1, 10, 3}), scores11 = shaped({1, 10, 11}), scores2 = shaped({2, 10, 10}), flat = shaped({10, 4});
        NonMaxSuppression op;
        CHECK(run(op, {&boxes3, &scores}) == "InvalidValue(\"`boxes` last dimension should have size 4\")");
        CHECK(run(op, {&boxes, &scores11}) == "IncompatibleInputShapes(\"`boxes` and `scores` have incompatible shapes\")");
        CHECK(run(op, {&boxes, &scores2}) == "IncompatibleInputShapes(\"`boxes` and `scores` have incompatible shapes\")");
        CHECK(run(op, {&boxes}) == "MissingInputs");
        CHECK(run(op, {&flat, &scores}) == "InputCastFailed(\"expected tensor with 3 dims\")");
        const Tensor iboxes = shaped({1, 10, 4}, DType::I32);
        CHECK(has(run(op, {&iboxes, &scores}), "InputCastFailed"));
        const Tensor two = host_scalar({2}, false, 1, 2), fcap = host_scalar({}, true, 1), icap = host_scalar({1}, false, 3), thr = host_scalar({1, 1}, true, 0.5), ithr = host_scalar({}, false, 1);
        CHECK(run(op, {&boxes, &scores, &two}) == "InputCastFailed(\"expected tensor with 0 dims\")"); // get_as: one element of any rank
        CHECK(has(run(op, {&boxes, &scores, &fcap}), "InputCastFailed(\"expected int32"));
        CHECK(has(run(op, {&boxes, &scores, &icap, &ithr}), "InputCastFailed(\"expected float32"));
        CHECK(has(run(op, {&boxes, &scores, nullptr, &thr, &ithr}), "InputCastFailed(\"expected float32"));
        CHECK(has(run(op, {&boxes, &scores, &icap, &thr, &thr, &thr}), "at most 5 inputs"));
        const Tensor dev_cap = shaped({1}, DType::I32), dev_thr = shaped({}, DType::F32); // no host value: device data
        msg = run(op, {&boxes, &scores, &dev_cap});
        CHECK(has(msg, "UnsupportedValue") && has(msg, "max_output_boxes_per_class must be a constant or computable from the input shapes (it depends on device data)"));
        msg = run(op, {&boxes, &scores, &icap, &dev_thr});
        CHECK(has(msg, "UnsupportedValue") && has(msg, "iou_threshold must be a constant"));
        msg = run(op, {&boxes, &scores, nullptr, nullptr, &dev_thr});
        CHECK(has(msg, "UnsupportedValue") && has(msg, "score_threshold must be a constant"));
        op.center_point_box = 2;
        CHECK(run(op, {&boxes, &scores, &icap, &thr, &thr}) == "InvalidValue(\"center_point_box must be 0 or 1\")");
    }

    // ---- a plan with the step: batch-coupled, reading back, and capture() refuses it FROM THE PLAN -- nothing runs, no capture begins (the context is never used)
    {
        onnx::Model g;
        for (const char *gi : {"boxes", "scores"}) { onnx::ValueInfo v; v.name = gi; v.elem_type = onnx::FLOAT; v.dims = {1, 4, 4}; v.dim_params = {"", "", ""}; g.inputs.push_back(v); }
        onnx::Node relu;
        relu.op_type = "Relu"; relu.name = "clip"; relu.inputs = {"scores"}; relu.outputs = {"scores_r"};
        onnx::Node nms;
        nms.op_type = "NonMaxSuppression"; nms.name = "post/nms"; nms.inputs = {"boxes", "scores_r"}; nms.outputs = {"selected"};
        g.nodes = {relu, nms};
        { onnx::ValueInfo v; v.name = "selected"; v.elem_type = onnx::INT64; g.outputs.push_back(v); }
        Graph plan(ctx, g, Graph::Options());
        CHECK(plan.batch_coupled_step() == "NonMaxSuppression \"post/nms\"");
        CHECK(plan.reading_back_step() == "NonMaxSuppression \"post/nms\"");
        msg = graph_error([&] { plan.capture({}); }); // (no feeds: a capture that got as far as its warm-up run would complain about the missing inputs instead)
        CHECK(has(msg, "capture: NonMaxSuppression \"post/nms\"") && has(msg, "a graph whose output shape depends on device values cannot be captured"));
        CHECK(!plan.captured());
        g.nodes = {relu};
        g.outputs[0].name = "scores_r";
        Graph plain(ctx, g, Graph::Options());
        CHECK(plain.reading_back_step().empty() && plain.batch_coupled_step().empty());
    }
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
