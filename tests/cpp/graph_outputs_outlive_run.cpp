// graph_outputs_outlive_run model.onnx inputs.safetensors outputs.safetensors
//
// Graph::run's contract: the tensors it returns own their storage.  rten_hip_run reads them back before anything else touches the context's buffer
// pool, so an output that still aliased a value of the finished run (a view handed out by a move instead of a copy) would go unnoticed there.  This
// program runs the graph once and then, BEFORE reading the outputs, takes buffers of every output's byte size from the pool and fills them: an output
// whose storage went back to the pool with the run is overwritten.  f32 inputs only; the outputs are written as a Safetensors file.
#include "rten_hip_graph.hpp"
#include "rten_hip_safetensors.hpp"

using namespace rten_hip;

int main(int argc, char **argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: graph_outputs_outlive_run model.onnx inputs.safetensors outputs.safetensors\n"); return 1; }
    try {
        const onnx::Model m = onnx::load(argv[1]);
        Context ctx(0);
        ctx.enable_pool();
        Graph g(ctx, m);
        const auto given = safetensors::read(argv[2]);
        std::vector<Tensor> feeds_store;
        Graph::Feeds feeds;
        feeds_store.reserve(g.inputs().size());
        for (auto &in : g.inputs()) {
            const safetensors::Entry &e = given.at(in.name);
            if (e.dtype != "F32") throw GraphError("input " + in.name + ": only F32 inputs are supported here");
            Tensor t(ctx, e.shape, DType::F32);
            if (t.bytes()) ctx.check(rten_hip_memcpy_h2d(ctx.raw(), t.ptr(), e.data.data(), t.bytes()));
            feeds_store.push_back(std::move(t));
            feeds.emplace_back(in.name, &feeds_store.back());
        }
        const std::vector<Tensor> outs = g.run(feeds);
        ctx.sync();
        {
            // The pool hands buffers out by exact byte size, last returned first.  A run returns at most one buffer per step output, so taking
            // (steps + 1) buffers of every output's size, all alive at once, empties the pool's list for that size: whatever the run left there
            // is handed out and filled.
            std::vector<Tensor> scribble;
            for (size_t round = 0; round < g.num_steps() + 1; round++)
                for (auto &o : outs) {
                    if (!o.bytes()) continue;
                    scribble.emplace_back(ctx, std::vector<int64_t>{(int64_t)o.bytes()}, DType::U8);
                    ctx.check(rten_hip_memset(ctx.raw(), scribble.back().ptr(), 0xA5, o.bytes()));
                }
            ctx.sync();
        }
        std::vector<std::pair<std::string, safetensors::Entry>> all;
        for (size_t i = 0; i < outs.size(); i++) {
            safetensors::Entry e;
            e.dtype = outs[i].dtype() == DType::F32 ? "F32" : outs[i].dtype() == DType::I32 ? "I32" : outs[i].dtype() == DType::U8 ? "U8" : "I8";
            e.shape = outs[i].shape();
            e.data.resize(outs[i].bytes());
            if (outs[i].bytes()) ctx.check(rten_hip_memcpy_d2h(ctx.raw(), &e.data[0], outs[i].ptr(), outs[i].bytes()));
            all.emplace_back(g.outputs()[i].name, std::move(e));
        }
        safetensors::write(argv[3], all);
        std::printf("ran %zu steps, saved %zu outputs\n", g.num_steps(), all.size());
        return 0;
    } catch (const OpError &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return e.kind == OpError::BackendUnavailable ? 2 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
