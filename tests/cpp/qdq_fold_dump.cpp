// Prints the canonical form's initializers of an ONNX model (include/rten_hip_graph.hpp, Graph::canonical_form): what the loader uploads after it has folded
// the DequantizeLinear nodes over initializers.  One line per initializer: name, ONNX element type, dims, the raw bytes in hex.  tests/test_qdq_ops.py compares
// the folded float32 initializers' bits with tests/qdq_rules.py.  A load error goes to stderr, exit status 1.  Needs no GPU.
#include <cstdio>

#include "rten_hip_graph.hpp"

using namespace rten_hip;

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: qdq_fold_dump model.onnx\n"); return 2; }
    try {
        const onnx::Model c = Graph::canonical_form(onnx::load(argv[1]));
        std::printf("folded %zu nodes %zu\n", c.folded_dequantize, c.nodes.size());
        for (auto &t : c.initializers) {
            std::printf("init %s %d [", t.name.c_str(), t.data_type);
            for (size_t i = 0; i < t.dims.size(); i++) std::printf("%s%lld", i ? "," : "", (long long)t.dims[i]);
            std::printf("] ");
            for (unsigned char b : t.raw) std::printf("%02x", b);
            std::printf("\n");
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
