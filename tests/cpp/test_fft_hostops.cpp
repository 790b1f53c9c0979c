// Host side of DFT and STFT in the C++ layers (include/rten_hip_ops.hpp, include/rten_hip_graph.hpp): attribute defaults and the opset-17 / opset-20 axis
// rule, what the loader refuses about the nodes, by node name -- the checks rten_hip_run --parse-only runs without a device --, registry membership, the
// operators' own input checks with the reference's strings, which refuse before anything touches the device (every Context here is a borrowed handle that is
// never dereferenced), batch coupling decided from the plan, and the host-only pass planner.  Needs no GPU.
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
static Tensor host_int(std::vector<int64_t> shape, int64_t v, size_t count = 1) {
    Tensor t = shaped(shape, DType::I32);
    auto h = std::make_shared<HostVal>();
    h->shape = std::move(shape);
    h->i.assign(count, v);
    t.set_host(h);
    return t;
}

int main() {
    // ---- the loader's reads and refusals, by node name
    onnx::Model m;
    for (const char *gi : {"x", "len_in", "axis_in", "step_in", "frame_in"}) { onnx::ValueInfo v; v.name = gi; m.inputs.push_back(v); }
    for (const char *c : {"len_c", "axis_c", "step_c", "window_c", "frame_c"}) { onnx::TensorProto t; t.name = c; m.initializers.push_back(t); }
    onnx::Node n;
    n.op_type = "DFT"; n.name = "spec/dft"; n.inputs = {"x"}; n.outputs = {"y"};
    m.opset = 17;
    Graph::DftNode a = Graph::read_dft_node(m, n, n.name);
    CHECK(!a.inverse && !a.onesided && a.axis_fixed && a.axis == 1); // before opset 20: the axis attribute, default 1
    m.opset = 19;
    CHECK(Graph::read_dft_node(m, n, n.name).axis == 1);
    m.opset = 20;
    a = Graph::read_dft_node(m, n, n.name);
    CHECK(!a.axis_fixed && a.axis == -2); // from opset 20: the optional third input, default -2
    n.inputs = {"x", "", "axis_c"};
    CHECK(!Graph::read_dft_node(m, n, n.name).axis_fixed);
    n.attrs = {int_attr("axis", 2), int_attr("inverse", 1), int_attr("onesided", 1)};
    a = Graph::read_dft_node(m, n, n.name);
    CHECK(a.inverse && a.onesided && a.axis_fixed && a.axis == 2); // an attribute, where the node has one, is the axis at every opset
    n.attrs.clear();
    n.inputs = {"x", "len_c", "axis_c", "len_c"};
    std::string msg = graph_error([&] { Graph::read_dft_node(m, n, n.name); });
    CHECK(has(msg, "DFT spec/dft") && has(msg, "takes at most 3 inputs (it has 4)"));
    n.inputs = {"x", "len_in"};
    msg = graph_error([&] { Graph::read_dft_node(m, n, n.name); });
    CHECK(has(msg, "DFT spec/dft") && has(msg, "dft_length must be a constant or computable from the input shapes") && has(msg, "\"len_in\""));
    n.inputs = {"x", "len_c", "axis_in"};
    msg = graph_error([&] { Graph::read_dft_node(m, n, n.name); });
    CHECK(has(msg, "DFT spec/dft") && has(msg, "axis must be a constant or computable from the input shapes") && has(msg, "\"axis_in\""));
    n.inputs = {};
    CHECK(has(graph_error([&] { Graph::read_dft_node(m, n, n.name); }), "the input is missing"));

    onnx::Node s;
    s.op_type = "STFT"; s.name = "front/stft"; s.inputs = {"x", "step_c", "window_c"}; s.outputs = {"y"};
    Graph::StftNode b = Graph::read_stft_node(m, s, s.name);
    CHECK(b.onesided && b.has_window && !b.has_frame_length); // onesided defaults to 1
    s.attrs = {int_attr("onesided", 0)};
    s.inputs = {"x", "step_c", "", "frame_c"};
    b = Graph::read_stft_node(m, s, s.name);
    CHECK(!b.onesided && !b.has_window && b.has_frame_length);
    s.inputs = {"x", "step_c"};
    msg = graph_error([&] { Graph::read_stft_node(m, s, s.name); });
    CHECK(has(msg, "STFT front/stft") && has(msg, "Either frame_length or window must be set"));
    s.inputs = {"x"};
    CHECK(has(graph_error([&] { Graph::read_stft_node(m, s, s.name); }), "the signal or frame_step input is missing"));
    s.inputs = {"x", "step_in", "window_c"};
    msg = graph_error([&] { Graph::read_stft_node(m, s, s.name); });
    CHECK(has(msg, "STFT front/stft") && has(msg, "frame_step must be a constant or computable from the input shapes") && has(msg, "\"step_in\""));
    s.inputs = {"x", "step_c", "window_c", "frame_in"};
    msg = graph_error([&] { Graph::read_stft_node(m, s, s.name); });
    CHECK(has(msg, "STFT front/stft") && has(msg, "frame_length must be a constant or computable from the input shapes") && has(msg, "\"frame_in\""));
    s.inputs = {"x", "step_c", "window_c", "frame_c", "frame_c"};
    CHECK(has(graph_error([&] { Graph::read_stft_node(m, s, s.name); }), "takes at most 4 inputs (it has 5)"));

    // ---- registry and operator defaults
    const OpRegistry reg = OpRegistry::with_all_ops();
    CHECK(reg.contains("DFT") && std::string(reg.create("DFT")->name()) == "DFT" && reg.create("DFT")->max_inputs() == 3);
    CHECK(reg.contains("STFT") && std::string(reg.create("STFT")->name()) == "STFT" && reg.create("STFT")->max_inputs() == 4);
    CHECK(!DFT().inverse && !DFT().onesided && STFT().onesided);

    // ---- the pass planner (host only)
    {
        int32_t r[16];
        CHECK(rten_hip_fft_plan(400, r, 16) == 4 && r[0] == 4 && r[1] == 4 && r[2] == 5 && r[3] == 5);
        CHECK(rten_hip_fft_plan(8, r, 16) == 2 && r[0] == 4 && r[1] == 2);
        CHECK(rten_hip_fft_plan(1, r, 16) == 0);
        CHECK(rten_hip_fft_plan(8191, r, 16) == 1 && r[0] == 8191);
        CHECK(rten_hip_fft_plan(RTEN_HIP_FFT_MAX + 1, r, 16) == -RTEN_HIP_ERR_UNSUPPORTED);
        CHECK(rten_hip_fft_plan(0, r, 16) == -RTEN_HIP_ERR_INVALID_VALUE && rten_hip_fft_plan(400, r, 3) == -RTEN_HIP_ERR_INVALID_VALUE);
    }

    alignas(16) static char no_device[64];
    Context ctx(reinterpret_cast<rten_hip_ctx *>(no_device), Context::Borrow{});
    // ---- the operators' own input checks: they throw before the context is used
    {
        auto run = [&](const Operator &op, std::vector<const Tensor *> in) { const InputList il(in.begin(), in.end()); return op_error([&] { op.run(ctx, il); }); };
        const Tensor real = shaped({1, 4, 1}), cplx = shaped({1, 4, 2}), three = shaped({1, 1, 3}), flat = shaped({4}), ints = shaped({1, 4, 1}, DType::I32);
        const Tensor zero = host_int({}, 0), minus1 = host_int({}, -1), two = host_int({2}, 1, 2), big = host_int({}, RTEN_HIP_FFT_MAX + 1), five = host_int({1}, 5);
        const Tensor dev = shaped({1}, DType::I32);
        DFT fwd, rfft, irfft;
        rfft.onesided = true;
        irfft.onesided = irfft.inverse = true;
        CHECK(run(fwd, {&flat}) == "InvalidValue(\"DFT input must have at least 2 dims\")");
        CHECK(run(fwd, {&three}) == "InvalidValue(\"Last dimension of DFT input must have size 1 or 2\")");
        CHECK(run(irfft, {&real}) == "InvalidValue(\"Inverse one-sided DFT (IRFFT) requires complex input\")");
        CHECK(run(rfft, {&cplx}) == "InvalidValue(\"DFT cannot be one-sided if input is complex\")");
        CHECK(run(fwd, {&cplx, nullptr, &minus1}) == "InvalidValue(\"DFT axis cannot be the complex dimension\")");
        CHECK(run(fwd, {&cplx, nullptr, &five}) == "InvalidValue(\"Axis is invalid\")");
        CHECK(run(fwd, {&real, &zero}) == "InvalidValue(\"dft_length must be >= 1\")");
        CHECK(run(fwd, {}) == "MissingInputs");
        CHECK(has(run(fwd, {&ints}), "InputCastFailed(\"expected float32"));
        CHECK(run(fwd, {&real, &two}) == "InputCastFailed(\"expected tensor with 0 dims\")");
        msg = run(fwd, {&real, &dev});
        CHECK(has(msg, "UnsupportedValue") && has(msg, "DFT: dft_length must be a constant or computable from the input shapes (it depends on device data)"));
        msg = run(fwd, {&real, nullptr, &dev});
        CHECK(has(msg, "UnsupportedValue") && has(msg, "DFT: axis must be a constant"));
        msg = run(fwd, {&real, &big});
        CHECK(has(msg, "UnsupportedValue") && has(msg, "DFT transform of length 8193 exceeds the limit of 8192 points (RTEN_HIP_FFT_MAX)"));

        const Tensor sig = shaped({1, 8}), sig3 = shaped({1, 8, 1}), csig = shaped({1, 8, 2}), sig4 = shaped({1, 8, 1, 1}), tsig = shaped({1, 8, 3}), window = shaped({4}), short_window = shaped({2});
        const Tensor four = host_int({}, 4), nine = host_int({}, 9), long_sig = shaped({1, 9000}), long_window = shaped({8193});
        STFT one, both;
        both.onesided = false;
        CHECK(run(one, {&sig4, &four, nullptr, &four}) == "InvalidValue(\"signal must have 2 or 3 dims\")");
        CHECK(run(one, {&sig, &four, nullptr, &zero}) == "InvalidValue(\"frame_length must be in range [1, signal_length]\")");
        CHECK(run(one, {&sig, &four, nullptr, &nine}) == "InvalidValue(\"frame_length must be in range [1, signal_length]\")");
        CHECK(run(one, {&sig, &zero, nullptr, &four}) == "InvalidValue(\"frame_step must be > 0\")");
        CHECK(run(one, {&sig, &four, &short_window, &four}) == "InvalidValue(\"window length must equal frame_length\")");
        CHECK(run(one, {&sig, &four}) == "InvalidValue(\"Either frame_length or window must be set\")");
        CHECK(run(both, {&tsig, &four, nullptr, &four}) == "InvalidValue(\"Last dimension of signal must have size 1 or 2\")");
        CHECK(run(one, {&csig, &four, &window}) == "InvalidValue(\"FFT cannot be one-sided if input is complex\")");
        CHECK(run(one, {&sig}) == "MissingInputs");
        msg = run(one, {&sig3, &dev, &window});
        CHECK(has(msg, "UnsupportedValue") && has(msg, "STFT: frame_step must be a constant"));
        msg = run(one, {&sig3, &four, &window, &dev});
        CHECK(has(msg, "UnsupportedValue") && has(msg, "STFT: frame_length must be a constant"));
        msg = run(one, {&long_sig, &four, &long_window});
        CHECK(has(msg, "UnsupportedValue") && has(msg, "STFT frame of length 8193 exceeds the limit of 8192 points (RTEN_HIP_FFT_MAX)"));
    }

    // ---- batch coupling, from the plan: a DFT along dim 0 couples the rows, STFT never does
    {
        onnx::Model g;
        g.opset = 17;
        { onnx::ValueInfo v; v.name = "x"; v.elem_type = onnx::FLOAT; v.dims = {4, 6, 1}; v.dim_params = {"", "", ""}; g.inputs.push_back(v); }
        onnx::Node d;
        d.op_type = "DFT"; d.name = "spec/dft"; d.inputs = {"x"}; d.outputs = {"y"}; d.attrs = {int_attr("axis", 0)};
        g.nodes = {d};
        { onnx::ValueInfo v; v.name = "y"; v.elem_type = onnx::FLOAT; g.outputs.push_back(v); }
        Graph along0(ctx, g, Graph::Options());
        CHECK(along0.batch_coupled_step() == "DFT \"spec/dft\"");
        g.nodes[0].attrs = {int_attr("axis", 1)};
        Graph along1(ctx, g, Graph::Options());
        CHECK(along1.batch_coupled_step().empty() && along1.reading_back_step().empty());
    }
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
