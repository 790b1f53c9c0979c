// Host side of RMSNormalization / SimplifiedLayerNormalization, SkipLayerNormalization / SkipSimplifiedLayerNormalization and the two RotaryEmbedding
// operators in the C++ layers (include/rten_hip_ops.hpp, include/rten_hip_graph.hpp): attribute defaults, registry names and domains, what the loader reads
// and refuses about the nodes, by node name -- the checks rten_hip_run --parse-only runs without a device --, the Add fusion decided from the model, the
// operators' own input checks with the reference's strings, which refuse before anything touches the device (every Context here is a borrowed handle that is
// never dereferenced), and the plan a graph of these nodes compiles to.  Needs no GPU; also built and run under -fsanitize=address,undefined.
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
    for (const char *gi : {"x", "skip", "pos"}) { onnx::ValueInfo v; v.name = gi; v.elem_type = std::strcmp(gi, "pos") ? onnx::FLOAT : onnx::INT64; m.inputs.push_back(v); }
    { onnx::ValueInfo v; v.name = "tokens"; v.elem_type = onnx::INT64; m.inputs.push_back(v); }
    for (const char *c : {"gamma", "beta", "bias", "cos", "sin"}) { onnx::TensorProto t; t.name = c; t.data_type = onnx::FLOAT; m.initializers.push_back(t); }
    { onnx::TensorProto t; t.name = "int_gamma"; t.data_type = onnx::INT32; m.initializers.push_back(t); }
    { onnx::ValueInfo v; v.name = "y"; v.elem_type = onnx::FLOAT; m.outputs.push_back(v); }

    onnx::Node n = make_node("RMSNormalization", "block/norm", {"x", "gamma"}, {"y"});
    CHECK(Graph::is_decoder_node(n));
    Graph::DecoderNode a = Graph::read_decoder_node(m, n, n.name);
    CHECK(!a.contrib && !a.rotary && !a.skip && a.rms && a.axis == -1 && !a.epsilon); // axis -1, epsilon left to the operator (1e-5)
    n.attrs = {int_attr("axis", -2), float_attr("epsilon", 1e-6f), int_attr("stash_type", 1)};
    a = Graph::read_decoder_node(m, n, n.name);
    CHECK(a.axis == -2 && a.epsilon && *a.epsilon == 1e-6f);
    n.attrs = {int_attr("stash_type", 0)};
    std::string msg = graph_error([&] { Graph::read_decoder_node(m, n, n.name); });
    CHECK(has(msg, "RMSNormalization block/norm") && has(msg, "stash_type = 0") && has(msg, "must be 1"));
    n.op_type = "SimplifiedLayerNormalization";
    msg = graph_error([&] { Graph::read_decoder_node(m, n, n.name); });
    CHECK(has(msg, "SimplifiedLayerNormalization block/norm") && has(msg, "stash_type = 0"));
    n.attrs.clear();
    CHECK(Graph::is_decoder_node(n) && Graph::read_decoder_node(m, n, n.name).rms);
    n.inputs = {"x", "int_gamma"};
    msg = graph_error([&] { Graph::read_decoder_node(m, n, n.name); });
    CHECK(has(msg, "block/norm") && has(msg, "input 1 (\"int_gamma\")") && has(msg, "float32 only"));
    n.inputs = {"tokens", "gamma"};
    CHECK(has(graph_error([&] { Graph::read_decoder_node(m, n, n.name); }), "input 0 (\"tokens\")"));
    n.inputs = {"x"};
    CHECK(has(graph_error([&] { Graph::read_decoder_node(m, n, n.name); }), "the X and scale inputs are required"));
    n.inputs = {"x", "gamma", "beta"};
    CHECK(has(graph_error([&] { Graph::read_decoder_node(m, n, n.name); }), "takes at most 2 inputs (it has 3)"));
    n.domain = MS; // SimplifiedLayerNormalization is registered in ai.onnx, not in com.microsoft
    CHECK(!Graph::is_decoder_node(n));

    onnx::Node s = make_node("SkipLayerNormalization", "block/skip", {"x", "skip", "gamma", "beta", "bias"}, {"y", "mean", "isv", "sum"}, MS);
    CHECK(Graph::is_decoder_node(s));
    msg = graph_error([&] { Graph::read_decoder_node(m, s, s.name); });
    CHECK(has(msg, "com.microsoft.SkipLayerNormalization block/skip") && has(msg, "the epsilon attribute is missing")); // required (onnx_registry.rs:1918-1922)
    s.attrs = {float_attr("epsilon", 1e-12f)};
    a = Graph::read_decoder_node(m, s, s.name);
    CHECK(a.contrib && a.skip && !a.rms && !a.rotary && *a.epsilon == 1e-12f && !a.want_sum); // named outputs nobody reads are fine, and the sum is not written
    m.nodes = {s, make_node("Identity", "reads_sum", {"sum"}, {"z"})};
    CHECK(Graph::read_decoder_node(m, s, s.name).want_sum);
    m.nodes = {s, make_node("Identity", "reads_mean", {"mean"}, {"z"})};
    msg = graph_error([&] { Graph::read_decoder_node(m, s, s.name); });
    CHECK(has(msg, "SkipLayerNormalization block/skip") && has(msg, "output 1 (mean, \"mean\") is read"));
    m.nodes = {s};
    { onnx::ValueInfo v; v.name = "isv"; m.outputs.push_back(v); }
    msg = graph_error([&] { Graph::read_decoder_node(m, s, s.name); });
    CHECK(has(msg, "output 2 (inv_std_var, \"isv\") is read")); // a graph output is a reader
    m.outputs.pop_back();
    s.outputs.push_back("fifth");
    CHECK(has(graph_error([&] { Graph::read_decoder_node(m, s, s.name); }), "has at most 4 outputs"));
    s.outputs.pop_back();
    s.op_type = "SkipSimplifiedLayerNormalization";
    CHECK(has(graph_error([&] { Graph::read_decoder_node(m, s, s.name); }), "takes at most 4 inputs (it has 5)")); // input, skip, gamma, bias?: no beta
    s.inputs = {"x", "skip", "gamma", "bias"};
    a = Graph::read_decoder_node(m, s, s.name);
    CHECK(a.skip && a.rms);
    s.inputs = {"x", "skip"};
    CHECK(has(graph_error([&] { Graph::read_decoder_node(m, s, s.name); }), "the input, skip and gamma inputs are required"));
    s.domain = ""; // the skip forms exist in com.microsoft only
    CHECK(!Graph::is_decoder_node(s));

    onnx::Node r = make_node("RotaryEmbedding", "attn/rope", {"x", "cos", "sin"}, {"y"});
    a = Graph::read_decoder_node(m, r, r.name);
    CHECK(a.rotary && !a.contrib && !a.interleaved && a.num_heads == 0 && a.rotary_embedding_dim == 0); // onnx_registry.rs:1832-1847
    r.attrs = {int_attr("interleaved", 1), int_attr("num_heads", 8), int_attr("rotary_embedding_dim", 32)};
    a = Graph::read_decoder_node(m, r, r.name);
    CHECK(a.interleaved && a.num_heads == 8 && a.rotary_embedding_dim == 32);
    r.inputs = {"x", "cos", "sin", "x"};
    msg = graph_error([&] { Graph::read_decoder_node(m, r, r.name); });
    CHECK(has(msg, "RotaryEmbedding attn/rope") && has(msg, "position_ids (\"x\")") && has(msg, "int32 / int64 only"));
    r.inputs = {"x", "cos", "sin", "pos"};
    CHECK(graph_error([&] { Graph::read_decoder_node(m, r, r.name); }).empty());
    r.inputs = {"x", "int_gamma", "sin"};
    CHECK(has(graph_error([&] { Graph::read_decoder_node(m, r, r.name); }), "input 1 (\"int_gamma\")"));
    r.inputs = {"x", "cos"};
    CHECK(has(graph_error([&] { Graph::read_decoder_node(m, r, r.name); }), "the X, cos_cache and sin_cache inputs are required"));
    r.domain = MS; // the contrib operator: X, position_ids, cos, sin
    r.attrs.clear();
    r.inputs = {"x", "pos", "cos", "sin"};
    a = Graph::read_decoder_node(m, r, r.name);
    CHECK(a.rotary && a.contrib && a.num_heads == 0); // num_heads absent: inferred from the cache when the operator runs
    r.inputs = {"x", "", "cos", "sin"};
    msg = graph_error([&] { Graph::read_decoder_node(m, r, r.name); });
    CHECK(has(msg, "com.microsoft.RotaryEmbedding attn/rope") && has(msg, "position_ids") && has(msg, "required"));
    r.inputs = {"x", "cos", "cos", "sin"};
    CHECK(has(graph_error([&] { Graph::read_decoder_node(m, r, r.name); }), "position_ids (\"cos\")"));
    r.attrs = {int_attr("num_heads", -1)};
    r.inputs = {"x", "pos", "cos", "sin"};
    CHECK(has(graph_error([&] { Graph::read_decoder_node(m, r, r.name); }), "must not be negative"));

    // ---- the Add an RMS node takes in, from the model alone
    {
        onnx::Model g;
        g.nodes = {make_node("Add", "residual", {"x", "skip"}, {"sum"}), make_node("MatMul", "other_reader", {"sum", "w"}, {"p"}),
                   make_node("RMSNormalization", "norm", {"sum", "gamma"}, {"y"})};
        CHECK(Graph::add_rms_consumer(g, 0) == 2 && Graph::add_rms_consumer(g, 1) == -1);
        g.nodes[2].attrs = {int_attr("axis", 1)}; // only the spelled-out last axis is known to be the last one at load
        CHECK(Graph::add_rms_consumer(g, 0) == -1);
        g.nodes[2].attrs.clear();
        g.nodes[2].inputs = {"gamma", "sum"}; // the sum must be the normalised operand
        CHECK(Graph::add_rms_consumer(g, 0) == -1);
        g.nodes[2].inputs = {"sum", "p"}; // a scale computed after the Add: the step could not run where the Add stood
        CHECK(Graph::add_rms_consumer(g, 0) == -1);
        g.nodes[2].inputs = {"sum", "gamma"};
        g.nodes[2].domain = MS;
        CHECK(Graph::add_rms_consumer(g, 0) == -1);
    }

    // ---- registry names and domains, operator defaults
    const OpRegistry reg = OpRegistry::with_all_ops();
    CHECK(reg.contains("RMSNormalization") && std::string(reg.create("RMSNormalization")->name()) == "RMSNormalization" && reg.create("RMSNormalization")->max_inputs() == 2);
    CHECK(reg.contains("SimplifiedLayerNormalization") && reg.create("SimplifiedLayerNormalization")->max_inputs() == 2);
    CHECK(reg.contains("RotaryEmbedding") && std::string(reg.create("RotaryEmbedding")->name()) == "RotaryEmbedding" && reg.create("RotaryEmbedding")->max_inputs() == 4);
    CHECK(reg.contains("com.microsoft.RotaryEmbedding") && std::string(reg.create("com.microsoft.RotaryEmbedding")->name()) == "com.microsoft.RotaryEmbedding");
    CHECK(reg.contains("com.microsoft.SkipLayerNormalization") && reg.create("com.microsoft.SkipLayerNormalization")->max_inputs() == 5);
    CHECK(reg.contains("com.microsoft.SkipSimplifiedLayerNormalization") && reg.create("com.microsoft.SkipSimplifiedLayerNormalization")->max_inputs() == 4);
    CHECK(std::string(reg.create("com.microsoft.SkipSimplifiedLayerNormalization")->name()) == "SkipSimplifiedLayerNormalisation"); // (sic, contrib.rs:192)
    CHECK(!reg.contains("SkipLayerNormalization") && !reg.contains("SkipSimplifiedLayerNormalization")); // not ai.onnx operators
    CHECK(RMSNormalization().axis == -1 && !RMSNormalization().epsilon && !RotaryEmbedding().interleaved && RotaryEmbedding().num_heads == 0 &&
          RotaryEmbeddingMicrosoft().rotary_embedding_dim == 0 && !SkipLayerNormalization().want_sum);

    alignas(16) static char no_device[64];
    Context ctx(reinterpret_cast<rten_hip_ctx *>(no_device), Context::Borrow{});
    // ---- the operators' own input checks: they throw before the context is used
    {
        auto run = [&](const Operator &op, std::vector<const Tensor *> in) { const InputList il(in.begin(), in.end()); return op_error([&] { op.run(ctx, il); }); };
        const Tensor x3 = shaped({2, 3, 4}), g4 = shaped({4}), g3 = shaped({3}), ints = shaped({2, 3, 4}, DType::I32);
        RMSNormalization rms;
        CHECK(run(rms, {&x3, &g3}) == "InvalidValue(\"`scale` is not broadcastable to normalized axes of input\")");
        CHECK(run(rms, {&x3}) == "MissingInputs");
        CHECK(has(run(rms, {&ints, &g4}), "InputCastFailed(\"expected float32"));
        rms.axis = 3;
        CHECK(run(rms, {&x3, &g4}) == "InvalidValue(\"Axis is invalid\")");
        rms.axis = -2;
        const Tensor row = shaped({1, 4});
        CHECK(has(run(rms, {&x3, &row}), "UnsupportedValue") && has(run(rms, {&x3, &row}), "already expanded"));

        SkipLayerNormalization sln;
        SkipSimplifiedLayerNormalization ssln;
        const Tensor x2 = shaped({2, 4}), s23 = shaped({2, 3}), x1 = shaped({4}), x4 = shaped({1, 1, 2, 4}), s124 = shaped({1, 2, 4}), s334 = shaped({3, 3, 4}), g14 = shaped({1, 4});
        for (const Operator *op : {(const Operator *)&sln, (const Operator *)&ssln}) {
            CHECK(run(*op, {&x2, &s23, &g4}) == "IncompatibleInputShapes(\"skip must broadcast to input over the batch dimension\")");
            CHECK(run(*op, {&x1, &x1, &g4}) == "InvalidValue(\"input must be 2 or 3 dimensioned\")");
            CHECK(run(*op, {&x4, &x4, &g4}) == "InvalidValue(\"input must be 2 or 3 dimensioned\")");
            CHECK(run(*op, {&x2, &x1, &g4}) == "InvalidValue(\"skip must be 2 or 3 dimensioned\")");
            CHECK(run(*op, {&x2, &s124, &g4}) == "IncompatibleInputShapes(\"skip must broadcast to input over the batch dimension\")");
            CHECK(run(*op, {&x3, &s334, &g4}) == "IncompatibleInputShapes(\"skip must broadcast to input over the batch dimension\")");
            CHECK(run(*op, {&x2, &x2, &g3}) == "InvalidValue(\"`scale` is not broadcastable to normalized axes of input\")");
            CHECK(run(*op, {&x2, &x2, &g14}) == "InputCastFailed(\"expected tensor with 1 dims\")");
            CHECK(run(*op, {&x2, &x2}) == "MissingInputs");
        }
        CHECK(run(sln, {&x2, &x2, &g4, &g3}) == "InvalidValue(\"`bias` is not broadcastable to normalized axes of input\")");

        RotaryEmbedding rope;
        const Tensor h8 = shaped({1, 2, 8}), h5 = shaped({1, 1, 5}), flat = shaped({2, 4}), c122 = shaped({1, 2, 2}), c22 = shaped({2, 2}), c121 = shaped({1, 2, 1}), c132 = shaped({1, 3, 2}),
                     c322 = shaped({3, 2, 2}), c124 = shaped({1, 2, 4}), c10 = shaped({1, 0}), one = shaped({1, 1, 1}), c111 = shaped({1, 1, 1});
        CHECK(run(rope, {&h8, &c124, &c124}) == "InvalidValue(\"num_heads must not be 0 for 3 dimensioned input\")");
        rope.num_heads = 2;
        CHECK(run(rope, {&h5, &c111, &c111}) == "InvalidValue(\"hidden_size must be divisible by num_heads\")");
        CHECK(run(rope, {&flat, &c122, &c122}) == "IncompatibleInputShapes(\"Input processed needs 3-4 dimensions\")");
        CHECK(run(rope, {&h8, &c22, &c22}) == "InvalidValue(\"cos/sin cache must be a 3D tensor\")");
        CHECK(run(rope, {&h8, &c121, &c122}) == "InvalidValue(\"Last dimension of cos cache does not match rotary_embedding_dim/2\")");
        CHECK(run(rope, {&h8, &c122, &c121}) == "InvalidValue(\"Last dimension of sin cache does not match rotary_embedding_dim/2\")");
        CHECK(run(rope, {&h8, &c132, &c132}) == "InvalidValue(\"cos/sin cache sequence length must be 1 or match the input\")");
        CHECK(run(rope, {&h8, &c322, &c322}) == "InvalidValue(\"cos/sin cache batch size must be 1 or match the input\")");
        rope.rotary_embedding_dim = 6;
        CHECK(run(rope, {&h8, &c122, &c122}) == "InvalidValue(\"rotary_embedding_dim must not exceed head size\")");
        rope.rotary_embedding_dim = 1;
        rope.num_heads = 1;
        CHECK(run(rope, {&one, &c10, &c10}) == "InvalidValue(\"rotary_embedding_dim must be a positive even number\")");
        rope.rotary_embedding_dim = 0;
        rope.num_heads = 2;
        const Tensor ids1d = shaped({2}, DType::I32), ids_f = shaped({1, 2}), far = host_ints({1, 2}, {0, 4}), near = host_ints({1, 2}, {0, -5});
        CHECK(run(rope, {&h8, &c22, &c22, &ids1d}) == "InputCastFailed(\"expected tensor with 2 dims\")");
        CHECK(has(run(rope, {&h8, &c22, &c22, &ids_f}), "InputCastFailed(\"expected int32"));
        const Tensor cache42 = shaped({4, 2});
        CHECK(run(rope, {&h8, &cache42, &cache42, &far}) == "InvalidValue(\"Entry in `indices` is out of range\")"); // host-known ids: Gather's message
        CHECK(run(rope, {&h8, &cache42, &cache42, &near}) == "InvalidValue(\"Entry in `indices` is out of range\")");

        RotaryEmbeddingMicrosoft ms;
        const Tensor x14 = shaped({1, 1, 4}), x16 = shaped({1, 1, 6}), ids11 = shaped({1, 1}, DType::I32), c11 = shaped({1, 1}), c12 = shaped({1, 2}), ids3 = shaped({1, 1, 1}, DType::I32);
        CHECK(run(ms, {&x14, &ids11, &c10, &c10}) == "InvalidValue(\"Last dimension of cos cache must not be 0\")");
        CHECK(run(ms, {&x16, &ids11, &c12, &c12}) == "InvalidValue(\"hidden_size must be divisible by head size\")");
        CHECK(run(ms, {&x14, &ids1d, &c12, &c12}) == "InvalidValue(\"position_ids must be a scalar, a 1-element vector or have 2 dims\")");
        CHECK(run(ms, {&x14, &ids3, &c12, &c12}) == "InvalidValue(\"position_ids must be a scalar, a 1-element vector or have 2 dims\")");
        CHECK(run(ms, {&flat, &ids11, &c12, &c12}) == "IncompatibleInputShapes(\"Input processed needs 3-4 dimensions\")");
        ms.rotary_embedding_dim = 2;
        CHECK(run(ms, {&x14, &ids11, &c11, &c11}) == "InvalidValue(\"num_heads must be specified when rotary_embedding_dim is set\")");
        ms.rotary_embedding_dim = 0;
        ms.num_heads = 2;
        const Tensor offset_far = host_ints({1}, {3}), x28 = shaped({1, 2, 8}); // positions 3 and 4 of a cache of 4
        CHECK(run(ms, {&x28, &offset_far, &cache42, &cache42}) == "InvalidValue(\"Entry in `indices` is out of range\")");
        CHECK(run(ms, {&x28, &ids11}) == "MissingInputs");
    }

    // ---- the plan: domains dispatch, the Add fusion is off without fusion, a normalisation over dim 0 couples the batch
    {
        onnx::Model g;
        g.opset = 23;
        for (const char *gi : {"x", "skip", "gamma", "cos", "sin", "offset"}) {
            onnx::ValueInfo v; v.name = gi; v.elem_type = std::strcmp(gi, "offset") ? onnx::FLOAT : onnx::INT64; g.inputs.push_back(v);
        }
        g.nodes = {make_node("Add", "residual", {"x", "skip"}, {"sum"}), make_node("RMSNormalization", "norm", {"sum", "gamma"}, {"n"}),
                   make_node("RotaryEmbedding", "rope", {"n", "offset", "cos", "sin"}, {"q"}, MS), make_node("RotaryEmbedding", "rope23", {"q", "cos", "sin"}, {"q2"}),
                   make_node("SkipSimplifiedLayerNormalization", "skip_norm", {"q2", "sum", "gamma"}, {"y", "", "", "res"}, MS)};
        g.nodes[4].attrs = {float_attr("epsilon", 1e-6f)};
        for (const char *o : {"y", "res"}) { onnx::ValueInfo v; v.name = o; v.elem_type = onnx::FLOAT; g.outputs.push_back(v); }
        Graph fused(ctx, g, Graph::Options());
        CHECK(fused.num_steps() == 4 && fused.num_fused_away() == 1);
        CHECK(has_step(fused, "Add+RMSNormalization:residual") && has_step(fused, "com.microsoft.RotaryEmbedding:rope") && has_step(fused, "RotaryEmbedding:rope23") &&
              has_step(fused, "SkipSimplifiedLayerNormalization:skip_norm"));
        CHECK(fused.batch_coupled_step().empty() && fused.reading_back_step().empty()); // nothing is read back: every step captures
        Graph::Options plain;
        plain.fuse = false;
        Graph unfused(ctx, g, plain);
        CHECK(unfused.num_steps() == 5 && unfused.num_fused_away() == 0 && has_step(unfused, "Add:residual") && has_step(unfused, "RMSNormalization:norm"));
        g.nodes[1].attrs = {int_attr("axis", 0)};
        Graph along0(ctx, g, Graph::Options());
        CHECK(along0.batch_coupled_step() == "RMSNormalization \"norm\"" && along0.num_fused_away() == 0);
        g.nodes[1].attrs = {int_attr("stash_type", 2)};
        CHECK(has(graph_error([&] { Graph refused(ctx, g, Graph::Options()); }), "RMSNormalization norm: stash_type = 2"));
        g.nodes[1].attrs.clear();
        g.nodes[4].domain = ""; // not an ai.onnx operator: the registry has no such name
        CHECK(has(graph_error([&] { Graph refused(ctx, g, Graph::Options()); }), "operator SkipSimplifiedLayerNormalization is not available on the HIP backend"));
        g.nodes[4].domain = "com.example";
        CHECK(has(graph_error([&] { Graph refused(ctx, g, Graph::Options()); }), "operator domain com.example is not supported"));
    }
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
