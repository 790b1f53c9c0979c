// Host side of com.microsoft GroupQueryAttention in the C++ layers (include/rten_hip_ops.hpp, include/rten_hip_graph.hpp): attribute defaults, the registry
// name, what the loader reads and refuses about the node, by node name -- the checks rten_hip_run --parse-only runs without a device --, the operator's own
// input checks with the reference's strings (src/ops/attention/contrib.rs:475-653), which refuse before anything touches the device (the Context here is
// a borrowed handle that is never dereferenced), and the plan a graph with the node compiles to.  Needs no GPU; also built and run under
// -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <string>

#include "rten_hip_graph.hpp"

using namespace rten_hip;
static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static onnx::Attr int_attr(const char *name, int64_t v) { onnx::Attr a; a.name = name; a.type = 2; a.i = v; return a; }
static onnx::Attr float_attr(const char *name, float v) { onnx::Attr a; a.name = name; a.type = 1; a.f = v; return a; }
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
static Tensor host_ints(std::vector<int64_t> shape, std::vector<int64_t> v) {
    Tensor t = shaped(shape, DType::I32);
    auto h = std::make_shared<HostVal>();
    h->shape = std::move(shape);
    h->i = std::move(v);
    t.set_host(h);
    return t;
}
static onnx::Node make_node(const char *op, const char *name, std::vector<std::string> in, std::vector<std::string> out, const char *domain = "") {
    onnx::Node n;
    n.op_type = op; n.name = name; n.inputs = std::move(in); n.outputs = std::move(out); n.domain = domain;
    return n;
}
static bool has_step(const Graph &g, const char *step) {
    for (auto &s : g.step_names()) if (s == step) return true;
    return false;
}

int main() {
    const char *MS = "com.microsoft";
    // ---- the loader's reads and refusals, by node name
    onnx::Model m;
    for (const char *gi : {"q", "k", "v", "past_k", "past_v", "bias", "sink"}) { onnx::ValueInfo v; v.name = gi; v.elem_type = onnx::FLOAT; m.inputs.push_back(v); }
    for (const char *gi : {"seqlens", "total", "pos"}) { onnx::ValueInfo v; v.name = gi; v.elem_type = std::strcmp(gi, "pos") ? onnx::INT32 : onnx::INT64; m.inputs.push_back(v); }
    { onnx::ValueInfo v; v.name = "float_lens"; v.elem_type = onnx::FLOAT; m.inputs.push_back(v); }
    { onnx::ValueInfo v; v.name = "int_q"; v.elem_type = onnx::INT32; m.inputs.push_back(v); }
    for (const char *c : {"cos", "sin"}) { onnx::TensorProto t; t.name = c; t.data_type = onnx::FLOAT; m.initializers.push_back(t); }
    for (const char *o : {"y", "pk"}) { onnx::ValueInfo v; v.name = o; v.elem_type = onnx::FLOAT; m.outputs.push_back(v); }

    const std::vector<std::string> base = {"q", "k", "v", "past_k", "past_v", "seqlens", "total"};
    onnx::Node n = make_node("GroupQueryAttention", "layer0/attn", base, {"y", "pk", "pv"}, MS);
    CHECK(Graph::is_gqa_node(n) && !Graph::is_decoder_node(n));
    CHECK(has(graph_error([&] { Graph::read_gqa_node(m, n, n.name); }), "com.microsoft.GroupQueryAttention layer0/attn: the num_heads and kv_num_heads attributes are required"));
    n.attrs = {int_attr("num_heads", 8), int_attr("kv_num_heads", 2)};
    Graph::GqaNode a = Graph::read_gqa_node(m, n, n.name);
    // defaults of the reference's reader (onnx_registry.rs:1467-1492): no scale, no rotary, window -1 (off), separate q / k / v; output 1 is a graph output
    CHECK(a.num_heads == 8 && a.kv_num_heads == 2 && !a.scale && !a.do_rotary && !a.rotary_interleaved && a.local_window_size == -1 && !a.packed && a.want_present);
    n.outputs = {"y"};
    CHECK(!Graph::read_gqa_node(m, n, n.name).want_present);
    n.outputs = {"y", "unread_k", "unread_v"};
    CHECK(!Graph::read_gqa_node(m, n, n.name).want_present); // named but unread
    n.attrs = {int_attr("num_heads", 8), int_attr("kv_num_heads", 2), float_attr("scale", 0.25f), int_attr("do_rotary", 1), int_attr("rotary_interleaved", 1),
               int_attr("local_window_size", 128)};
    n.inputs = {"q", "", "", "past_k", "past_v", "seqlens", "total", "cos", "sin", "pos", "bias"};
    a = Graph::read_gqa_node(m, n, n.name);
    CHECK(a.scale && *a.scale == 0.25f && a.do_rotary && a.rotary_interleaved && a.local_window_size == 128 && a.packed);
    n.inputs = {"q", "", "", "past_k", "past_v", "seqlens", "total"};
    CHECK(has(graph_error([&] { Graph::read_gqa_node(m, n, n.name); }), "layer0/attn: cos_cache and sin_cache are required when do_rotary is set"));
    n.inputs = base;
    auto with = [&](std::vector<onnx::Attr> extra) {
        n.attrs = {int_attr("num_heads", 8), int_attr("kv_num_heads", 2)};
        for (auto &e : extra) n.attrs.push_back(e);
        return graph_error([&] { Graph::read_gqa_node(m, n, n.name); });
    };
    CHECK(has(with({int_attr("smooth_softmax", 1)}), "layer0/attn: smooth_softmax is not supported"));
    CHECK(has(with({float_attr("softcap", 30.f)}), "layer0/attn: softcap != 0 is not supported"));
    CHECK(with({float_attr("softcap", 0.f), int_attr("smooth_softmax", 0)}).empty());
    n.attrs = {int_attr("num_heads", 3), int_attr("kv_num_heads", 2)};
    CHECK(has(graph_error([&] { Graph::read_gqa_node(m, n, n.name); }), "num_heads must be a multiple of kv_num_heads"));
    n.attrs = {int_attr("num_heads", 0), int_attr("kv_num_heads", 2)};
    CHECK(has(graph_error([&] { Graph::read_gqa_node(m, n, n.name); }), "num_heads and kv_num_heads must be positive"));
    n.attrs = {int_attr("num_heads", 8), int_attr("kv_num_heads", 2)};
    n.inputs = {"q", "k", "v", "past_k", "past_v", "seqlens", "total", "", "", "", "", "sink"};
    CHECK(has(graph_error([&] { Graph::read_gqa_node(m, n, n.name); }), "layer0/attn: the head_sink input (\"sink\") is not supported"));
    for (size_t extra = 12; extra < 16; extra++) {
        n.inputs = base;
        n.inputs.resize(extra, "");
        n.inputs.push_back("bias");
        const std::string msg = graph_error([&] { Graph::read_gqa_node(m, n, n.name); });
        CHECK(has(msg, "layer0/attn: input ") && has(msg, "inputs 12-15"));
    }
    n.inputs = base;
    n.outputs = {"y", "pk", "pv", "qk"};
    CHECK(has(graph_error([&] { Graph::read_gqa_node(m, n, n.name); }), "layer0/attn: output 3 (output_qk, \"qk\") is not supported"));
    n.outputs = {"y", "pk", "pv"};
    n.inputs = {"int_q", "k", "v", "past_k", "past_v", "seqlens", "total"};
    CHECK(has(graph_error([&] { Graph::read_gqa_node(m, n, n.name); }), "input 0 (\"int_q\") has element type 6: float32 only"));
    n.inputs = {"q", "k", "v", "past_k", "past_v", "float_lens", "total"};
    CHECK(has(graph_error([&] { Graph::read_gqa_node(m, n, n.name); }), "input 5 (\"float_lens\") has element type 1: int32 / int64 only"));
    n.inputs = {"q", "k", "", "past_k", "past_v", "seqlens", "total"};
    CHECK(has(graph_error([&] { Graph::read_gqa_node(m, n, n.name); }), "key and value must both be present or both absent"));
    n.inputs = {"q", "k", "v", "past_k", "", "seqlens", "total"};
    CHECK(has(graph_error([&] { Graph::read_gqa_node(m, n, n.name); }), "past_key and past_value must both be present or both absent"));
    n.inputs = {"q", "k", "v", "past_k", "past_v", "seqlens"};
    CHECK(has(graph_error([&] { Graph::read_gqa_node(m, n, n.name); }), "the query, seqlens_k and total_sequence_length inputs are required"));

    // ---- registry and the operator's defaults
    const OpRegistry reg = OpRegistry::with_all_ops();
    CHECK(reg.contains("com.microsoft.GroupQueryAttention") && !reg.contains("GroupQueryAttention"));
    CHECK(reg.create("com.microsoft.GroupQueryAttention")->max_inputs() == 12 && std::string(reg.create("com.microsoft.GroupQueryAttention")->name()) == "com.microsoft.GroupQueryAttention");
    {
        GroupQueryAttention d;
        CHECK(!d.scale && !d.do_rotary && !d.rotary_interleaved && d.local_window_size == -1 && d.softcap == 0.f && !d.smooth_softmax && d.want_present);
    }

    alignas(16) static char no_device[64];
    Context ctx(reinterpret_cast<rten_hip_ctx *>(no_device), Context::Borrow{});
    // ---- the operator's own input checks: they throw before the context is used
    {
        auto run = [&](const Operator &op, std::vector<const Tensor *> in) { const InputList il(in.begin(), in.end()); return op_error([&] { op.run(ctx, il); }); };
        GroupQueryAttention op;
        op.num_heads = 2; op.kv_num_heads = 1;
        const Tensor q = shaped({1, 2, 16}), k = shaped({1, 2, 8}), v = shaped({1, 2, 8}), one = host_ints({1}, {1}), two = host_ints({}, {2});
        const Tensor dev_lens = shaped({1}, DType::I32), dev_total = shaped({}, DType::I32);
        CHECK(run(op, {&q, &k, &v, nullptr, nullptr, &one}) == "MissingInputs");
        const Tensor k2 = shaped({2, 2, 8}), v16 = shaped({1, 2, 16}), k3 = shaped({1, 3, 8}), packed_bad = shaped({1, 2, 30}), flat = shaped({2, 16});
        CHECK(run(op, {&flat, &k, &v, nullptr, nullptr, &one, &two}) == "InputCastFailed(\"expected tensor with 3 dims\")");
        CHECK(run(op, {&q, &k2, &k2, nullptr, nullptr, &one, &two}) == "IncompatibleInputShapes(\"key and value batch size must match query\")");
        CHECK(run(op, {&q, &k, &v16, nullptr, nullptr, &one, &two}) == "IncompatibleInputShapes(\"key and value must have the same shape\")");
        CHECK(run(op, {&q, &v16, &v16, nullptr, nullptr, &one, &two}) == "IncompatibleInputShapes(\"key hidden size must equal kv_num_heads * head_size\")");
        CHECK(run(op, {&q, &k3, &k3, nullptr, nullptr, &one, &two}) == "UnsupportedValue(\"key sequence length must match query sequence length\")");
        CHECK(run(op, {&packed_bad, nullptr, nullptr, nullptr, nullptr, &one, &two}) == "IncompatibleInputShapes(\"packed query hidden size must be divisible by num_heads + 2 * kv_num_heads\")");
        CHECK(run(op, {&q, &k, nullptr, nullptr, nullptr, &one, &two}) == "InvalidValue(\"key and value must both be present or both absent\")");
        const Tensor lens2 = host_ints({2}, {1, 1}), lens12 = host_ints({1, 2}, {1, 1}), zero = host_ints({}, {0}), float_total = shaped({});
        CHECK(run(op, {&q, &k, &v, nullptr, nullptr, &lens2, &two}) == "IncompatibleInputShapes(\"seqlens_k must have batch_size elements\")");
        CHECK(run(op, {&q, &k, &v, nullptr, nullptr, &lens12, &two}) == "UnsupportedValue(\"seqlens_k must be a vector\")");
        CHECK(run(op, {&q, &k, &v, nullptr, nullptr, &one, &zero}) == "InvalidValue(\"total_sequence_length must be positive\")");
        CHECK(has(run(op, {&q, &k, &v, nullptr, nullptr, &one, &float_total}), "InputCastFailed(\"expected int32"));
        const Tensor past2 = shaped({1, 1, 2, 8}), past3 = shaped({1, 1, 3, 8}), three = host_ints({1}, {3}), four = host_ints({}, {4});
        CHECK(run(op, {&q, &k, &v, &past2, &past3, &three, &four}) == "IncompatibleInputShapes(\"past_key/past_value shape does not match\")");
        CHECK(run(op, {&q, &k, &v, &past2, nullptr, &three, &four}) == "InvalidValue(\"past_key and past_value must both be present or both absent\")");
        const Tensor q2 = shaped({2, 2, 16}), kk2 = shaped({2, 2, 8}), past22 = shaped({2, 1, 2, 8}), lens33 = host_ints({2}, {3, 3});
        CHECK(run(op, {&q2, &kk2, &kk2, &past22, &past22, &lens33, &four}) == "UnsupportedValue(\"batch size must be 1 when sequence_length > 1 and a past context is given\")");
        // the three value errors of host-known seqlens_k (contrib.rs:630-639)
        const Tensor lens0 = host_ints({1}, {0}), tot1 = host_ints({}, {1}), nine = host_ints({1}, {9}), ten = host_ints({}, {10}), neg = host_ints({1}, {-1});
        const Tensor q1 = shaped({1, 1, 16}), k1 = shaped({1, 1, 8});
        CHECK(run(op, {&q, &k, &v, nullptr, nullptr, &lens0, &tot1}) == "InvalidValue(\"seqlens_k entry is too small for the query sequence length\")");
        CHECK(run(op, {&q, &k, &v, nullptr, nullptr, &lens0, &two}) == "InvalidValue(\"seqlens_k entry is too small for the query sequence length\")");
        CHECK(run(op, {&q1, &k1, &k1, &past2, &past2, &nine, &ten}) == "InvalidValue(\"seqlens_k entry is out of range\")");
        CHECK(run(op, {&q, &k, &v, nullptr, nullptr, &neg, &two}) == "InvalidValue(\"seqlens_k entry is out of range\")");
        for (std::vector<int64_t> s : {std::vector<int64_t>{1, 1, 1, 2}, {1, 1, 2, 1}, {1, 3, 2, 2}}) {
            const Tensor bias = shaped(s);
            CHECK(run(op, {&q, &k, &v, nullptr, nullptr, &one, &two, nullptr, nullptr, nullptr, &bias}) == "IncompatibleInputShapes(\"attention_bias shape is incompatible with query/key shapes\")");
        }
        const Tensor sink = shaped({2});
        CHECK(run(op, {&q, &k, &v, nullptr, nullptr, &one, &two, nullptr, nullptr, nullptr, nullptr, &sink}) == "UnsupportedValue(\"head_sink is not supported\")");
        op.do_rotary = true;
        CHECK(run(op, {&q, &k, &v, nullptr, nullptr, &one, &two}) == "InvalidValue(\"cos_cache and sin_cache are required when do_rotary is set\")");
        const Tensor wide = shaped({4, 8}), cache = shaped({4, 2}), far = host_ints({1, 2}, {0, 4});
        CHECK(run(op, {&q, &k, &v, nullptr, nullptr, &one, &two, &wide, &wide}) == "InvalidValue(\"rotary_embedding_dim must not exceed head size\")");
        CHECK(run(op, {&q, &k, &v, nullptr, nullptr, &one, &two, &cache, &cache, &far}) == "InvalidValue(\"Entry in `indices` is out of range\")");
        op.do_rotary = false;
        op.smooth_softmax = true;
        CHECK(run(op, {&q, &k, &v, nullptr, nullptr, &one, &two}) == "UnsupportedValue(\"smooth_softmax is not supported\")");
        op.smooth_softmax = false;
        op.softcap = 30.f;
        CHECK(run(op, {&q, &k, &v, nullptr, nullptr, &one, &two}) == "UnsupportedValue(\"softcap is not supported\")");
        op.softcap = 0.f;
        op.num_heads = 3; op.kv_num_heads = 2;
        CHECK(run(op, {&q, &k, &v, nullptr, nullptr, &dev_lens, &dev_total}) == "InvalidValue(\"num_heads must be a multiple of kv_num_heads\")");
        op.num_heads = 3; op.kv_num_heads = 1;
        CHECK(run(op, {&q, &k, &v, nullptr, nullptr, &dev_lens, &dev_total}) == "IncompatibleInputShapes(\"query hidden size must be divisible by num_heads\")");
    }

    // ---- the plan: the node is one step under its domain's name, reads nothing back (it captures) and does not couple the batch
    {
        onnx::Model g;
        g.opset = 21;
        for (const char *gi : {"x", "wq", "wk", "wv", "past_k", "past_v", "cos", "sin"}) { onnx::ValueInfo v; v.name = gi; v.elem_type = onnx::FLOAT; g.inputs.push_back(v); }
        for (const char *gi : {"seqlens", "total"}) { onnx::ValueInfo v; v.name = gi; v.elem_type = onnx::INT32; g.inputs.push_back(v); }
        g.nodes = {make_node("MatMul", "q_proj", {"x", "wq"}, {"q"}), make_node("MatMul", "k_proj", {"x", "wk"}, {"k"}), make_node("MatMul", "v_proj", {"x", "wv"}, {"v"}),
                   make_node("GroupQueryAttention", "attn", {"q", "k", "v", "past_k", "past_v", "seqlens", "total", "cos", "sin"}, {"y", "present_k", "present_v"}, MS)};
        g.nodes[3].attrs = {int_attr("num_heads", 4), int_attr("kv_num_heads", 2), int_attr("do_rotary", 1)};
        for (const char *o : {"y", "present_k", "present_v"}) { onnx::ValueInfo v; v.name = o; v.elem_type = onnx::FLOAT; g.outputs.push_back(v); }
        for (bool fuse : {true, false}) {
            Graph::Options opt;
            opt.fuse = fuse;
            Graph plan(ctx, g, opt);
            CHECK(plan.num_steps() == 4 && has_step(plan, "com.microsoft.GroupQueryAttention:attn"));
            CHECK(plan.batch_coupled_step().empty() && plan.reading_back_step().empty());
        }
        g.nodes[3].attrs.push_back(int_attr("smooth_softmax", 1));
        CHECK(has(graph_error([&] { Graph refused(ctx, g, Graph::Options()); }), "com.microsoft.GroupQueryAttention attn: smooth_softmax is not supported"));
        g.nodes[3].attrs.pop_back();
        g.nodes[3].domain = ""; // not an ai.onnx operator
        CHECK(has(graph_error([&] { Graph refused(ctx, g, Graph::Options()); }), "operator GroupQueryAttention is not available on the HIP backend"));
    }
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
