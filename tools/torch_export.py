"""ONNX files written by PyTorch's own exporter, without the `onnx` python package (absent in this image).

`torch.onnx.export` refuses to run without `onnx`, but that package is only used for post-processing: the TorchScript
exporter's graph passes and the protobuf serialiser are C++ inside torch.  `export_bytes` drives them directly
(`_model_to_graph` + `Graph._export_onnx`, the calls `torch.onnx.export` makes itself), so the tests can feed
`rten_hip_run` / `include/rten_hip_graph.hpp` REAL exporter output -- node naming, initializer layout, BN folding, Gemm /
Flatten / Shape idioms as PyTorch emits them -- next to the graphs `rten_amd/onnx_writer.py` manufactures.

Test and tooling infrastructure only: nothing under rten_amd/ imports this.
    python tools/torch_export.py resnet50 /tmp/resnet50_torch.onnx     # BASELINE topology, the harness's synthetic weights
    python tools/torch_export.py encoder /tmp/bert_base_torch.onnx     # BERT-base sized encoder in plain torch.nn, batch 32 x 128
    python tools/torch_export.py bert /tmp/bert_torch.onnx             # transformers.BertModel, random init, 2 layers (its mask
                                                                       # subgraph needs NonZero / Where / Expand: not loadable yet)
    python tools/torch_export.py mobile /tmp/mobile_torch.onnx         # small MobileNetV2 / V3 / EfficientNet-style network (activations)
    python tools/torch_export.py yolo /tmp/yolo_torch.onnx             # small YOLOv8-style detector (Split, Resize, SPPF, DFL head)
    python tools/torch_export.py classifier_topk /tmp/cls_topk.onnx    # the mobile network + softmax(-1) + topk(5)
    python tools/torch_export.py segment_argmax /tmp/seg_argmax.onnx   # mobile features + class conv + bilinear interpolate + argmax(1)
    python tools/torch_export.py yolo_filter /tmp/yolo_filter.onnx     # the detector + scores.max(1) + topk over anchors + Gather by index
    python tools/torch_export.py recognizer_gru /tmp/rec_gru.onnx      # text-recogniser shape: Conv2d + ReLU, columns as time steps, bidirectional
    python tools/torch_export.py recognizer_lstm /tmp/rec_lstm.onnx    #   GRU / LSTM, Linear head (dynamic batch and width)
    python tools/torch_export.py recognizer_ctc /tmp/rec_ctc.onnx      # the GRU recogniser with its log_softmax head (LogSoftmax)
    python tools/torch_export.py generator /tmp/generator.onnx         # image-to-image generator: Conv / InstanceNorm2d / ReLU, residual blocks, ConvTranspose, Tanh
    python tools/torch_export.py preact /tmp/preact.onnx               # pre-activation blocks (BN -> ReLU -> Conv): BatchNormalization nodes that survive export
    python tools/torch_export.py reflect_generator /tmp/rgen.onnx      # the generator with ReflectionPad2d / ReplicationPad2d / F.pad (Pad nodes) and nn.PReLU
    python tools/torch_export.py gpt2_mlp /tmp/gpt2_mlp.onnx           # LayerNorm, Linear, gelu_new written out with torch.pow(x, 3.0), Linear
    python tools/torch_export.py box_decode /tmp/box_decode.onnx       # conv head + anchor decode: Exp, Min / Max against the image bounds, Sqrt, Reciprocal, Neg, Abs
    python tools/torch_export.py embedding_head /tmp/embed.onnx         # small encoder + masked mean pooling + F.normalize (ReduceL2), dynamic batch / sequence
    python tools/torch_export.py reduce_zoo /tmp/reduce_zoo.onnx        # ReduceL1 / ReduceLogSumExp / two-axis ReduceL2 / ReduceProd as the exporter writes them
    python tools/torch_export.py warp /tmp/warp.onnx                    # Conv features warped by F.grid_sample along a predicted flow (GridSample), dynamic batch
    python tools/torch_export.py pixel_shuffle_sr /tmp/sr.onnx          # Conv / ReLU / Conv / nn.PixelShuffle (Reshape / 6-D Transpose / Reshape)
    python tools/torch_export.py roberta /tmp/roberta.onnx              # transformers.RobertaModel, 1 small layer: position ids by CumSum, buffered token_type_ids by GatherElements
    python tools/torch_export.py causal_decoder /tmp/decoder.onnx       # embeddings + one causal attention block in plain torch.nn: CumSum, Trilu, GatherElements, Tile
    python tools/torch_export.py dynamic_upsample /tmp/dyn_up.onnx     # F.interpolate(scale_factor=2) with dynamic H / W as Shape -> .. -> Floor -> .. -> Resize(sizes), written with onnx_writer
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


_INDEX_SYMBOLICS_REGISTERED = False


def _register_index_symbolics():
    """cumsum -> CumSum, gather -> GatherElements, triu / tril -> Trilu, as custom symbolics.  PyTorch has them in its symbolic_opset11 / symbolic_opset14 modules,
    which the exporter does not load on its own (without them torch.cumsum fails with "ONNX export of cumsum in opset 9").  Importing those modules whole would also
    change how every OTHER operator exports from then on, for the rest of the process (hardswish becomes a HardSwish node, pixel_shuffle a DepthToSpace node, ...), and
    with it the graphs the existing builders here are known to produce; so only these four are registered, with the bodies PyTorch gives them."""
    global _INDEX_SYMBOLICS_REGISTERED
    if _INDEX_SYMBOLICS_REGISTERED:
        return
    import torch
    from torch.onnx._internal.torchscript_exporter import symbolic_helper as SH

    @SH.parse_args("v", "i", "none")
    def cumsum(g, self, dim, dtype=None):
        return g.op("CumSum", self, g.op("Constant", value_t=torch.tensor(dim, dtype=torch.int)))

    @SH.parse_args("v", "i", "v", "v")
    def gather(g, self, dim, index, sparse_grad=False):
        if SH._maybe_get_const(sparse_grad, "i"):
            return SH._unimplemented("gather", "sparse_grad == True")
        return g.op("GatherElements", self, index, axis_i=dim)

    def triu(g, self, diagonal, out=None):
        return g.op("Trilu", self, diagonal, upper_i=1)

    def tril(g, self, diagonal, out=None):
        return g.op("Trilu", self, diagonal, upper_i=0)

    torch.onnx.register_custom_op_symbolic("aten::cumsum", cumsum, 11)
    torch.onnx.register_custom_op_symbolic("aten::gather", gather, 11)
    torch.onnx.register_custom_op_symbolic("aten::triu", triu, 14)
    torch.onnx.register_custom_op_symbolic("aten::tril", tril, 14)
    _INDEX_SYMBOLICS_REGISTERED = True


_STFT_SYMBOLIC_REGISTERED = False


def _register_stft_symbolic():
    """aten::stft -> STFT, as a custom symbolic.  PyTorch has it in its symbolic_opset17 module, which the exporter does not load on its own (without it
    torch.stft fails with "ONNX export of stft in opset 9"), and importing that module whole would change how other operators export for the rest of the process
    (layer_norm becomes a LayerNormalization node, ...): the reason _register_index_symbolics gives.  So only this one is registered, with the body PyTorch
    gives it for what the builders here use: a [batch, signal] input and a window of n_fft values.  frame_step and frame_length are int64 Constants, the
    window is Cast to the signal's type, and the [batch, frames, bins, 2] result is transposed to torch.stft's [batch, bins, frames, 2]."""
    global _STFT_SYMBOLIC_REGISTERED
    if _STFT_SYMBOLIC_REGISTERED:
        return
    import torch
    from torch.onnx._internal.torchscript_exporter import symbolic_helper as SH

    @SH.parse_args("v", "i", "i", "i", "v", "b", "b", "b", "b")
    def stft(g, input, n_fft, hop_length=None, win_length=None, window=None, normalized=False, onesided=True, return_complex=False, align_to_window=None):
        if return_complex:
            return SH._unimplemented("stft", "complex types")
        if align_to_window is not None:
            return SH._unimplemented("stft", "the align_to_window option")
        if SH._get_tensor_rank(input) != 2 or SH._is_none(window) or SH._get_tensor_dim_size(window, dim=0) != n_fft:
            return SH._unimplemented("stft", "anything but a [batch, signal] input with a window of n_fft values")
        frame_step = g.op("Constant", value_t=torch.tensor(hop_length if hop_length is not None else n_fft // 4, dtype=torch.int64))
        frame_length = g.op("Constant", value_t=torch.tensor(n_fft, dtype=torch.int64))
        window = g.op("Cast", window, to_i=1)  # (FLOAT: the signal's type)
        result = g.op("STFT", input, frame_step, window, frame_length, onesided_i=1 if onesided is None or onesided else 0)
        result = g.op("Transpose", result, perm_i=[0, 2, 1, 3])
        if normalized:
            result = g.op("Div", result, g.op("Constant", value_t=torch.sqrt(torch.tensor(n_fft, dtype=torch.float32))))
        return result

    torch.onnx.register_custom_op_symbolic("aten::stft", stft, 17)
    _STFT_SYMBOLIC_REGISTERED = True


def export_bytes(model, args, input_names, output_names, dynamic_axes=None, opset: int = 17) -> bytes:
    import torch
    import torch.onnx._internal.torchscript_exporter.utils as TU
    import torch.onnx._internal.torchscript_exporter.symbolic_opset16  # noqa: F401  (registers grid_sampler -> GridSample; without it F.grid_sample is UnsupportedOperatorError)
    _register_index_symbolics()
    _register_stft_symbolic()
    from torch.onnx._internal.torchscript_exporter._globals import GLOBALS
    warnings.filterwarnings("ignore")
    GLOBALS.export_onnx_opset_version = opset
    model.eval()
    ONNX = torch.onnx.OperatorExportTypes.ONNX
    with torch.no_grad(), TU.exporter_context(model, torch.onnx.TrainingMode.EVAL, False):
        graph, params, _ = TU._model_to_graph(model, args, verbose=False, input_names=input_names, output_names=output_names,
                                              operator_export_type=ONNX, do_constant_folding=True, dynamic_axes=dynamic_axes or {})
        proto, _, _, _ = graph._export_onnx(params, opset, dynamic_axes or {}, False, ONNX, True, False, {}, True, "", {})
    return proto


def resnet50_module(weights):
    """ResNet-50 v1.5 as torchvision / timm lay it out, BatchNorm already folded (Conv2d with bias), parameters taken from
    rten_amd.workloads.resnet50.make_weights() so the oracle can run the same network."""
    import torch
    import torch.nn as nn
    from rten_amd.workloads import resnet50 as R

    specs = {l["name"]: l for l in R.conv_specs()}

    def conv(name):
        l = specs[name]
        c = nn.Conv2d(l["cin"], l["cout"], l["k"], stride=l["stride"], padding=l["pad"], bias=True)
        c.weight.data = torch.from_numpy(weights[name][0].copy())
        c.bias.data = torch.from_numpy(weights[name][1].copy())
        return c

    class Bottleneck(nn.Module):
        def __init__(self, pre, first):
            super().__init__()
            self.conv1, self.conv2, self.conv3 = conv(pre + "c1"), conv(pre + "c2"), conv(pre + "c3")
            self.downsample = conv(pre + "ds") if first else None

        def forward(self, x):
            idn = x if self.downsample is None else self.downsample(x)
            y = torch.relu(self.conv1(x))
            y = torch.relu(self.conv2(y))
            return torch.relu(self.conv3(y) + idn)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.stem = conv("stem")
            self.pool = nn.MaxPool2d(3, stride=2, padding=1)
            self.blocks = nn.Sequential(*[Bottleneck(f"s{si}b{bi}", bi == 0) for si, (_, n, _) in enumerate(R.STAGES) for bi in range(n)])
            self.fc = nn.Linear(2048, weights["fc"][0].shape[0])
            self.fc.weight.data = torch.from_numpy(weights["fc"][0].copy())
            self.fc.bias.data = torch.from_numpy(weights["fc"][1].copy())

        def forward(self, x):
            y = self.blocks(self.pool(torch.relu(self.stem(x))))
            return self.fc(torch.flatten(nn.functional.adaptive_avg_pool2d(y, 1), 1))

    return Net().eval()


def resnet50_onnx(weights, image: int = 224) -> bytes:
    import torch
    return export_bytes(resnet50_module(weights), (torch.zeros(2, 3, image, image),), ["x"], ["logits"], {"x": {0: "batch"}, "logits": {0: "batch"}})


def encoder_module(cfg, w, seq, dynamic_seq=False):
    """A BERT encoder in plain torch.nn (Embedding, Linear, LayerNorm, GELU, matmul / softmax attention with an additive
    mask) holding rten_amd.workloads.bert.make_weights(cfg): the operator order of oracle.models.bert_forward.  PyTorch's
    exporter writes nn.LayerNorm as ReduceMean / Sub / Pow / Sqrt / Div / Mul / Add and nn.GELU as Div / Erf / Add / Mul / Mul,
    Linear as MatMul + Add, scalars as Constant nodes.  dynamic_seq: the position ids are sliced to the input's sequence length (a Shape -> Gather -> Slice
    chain in the export) instead of being a [1, seq] constant, so that the file can be exported with a dynamic sequence axis."""
    import math
    import torch
    import torch.nn as nn

    def lin(wm, b):
        l = nn.Linear(wm.shape[0], wm.shape[1])
        l.weight.data, l.bias.data = torch.from_numpy(np.ascontiguousarray(wm.T)), torch.from_numpy(b.copy())
        return l

    def ln(g, b):
        l = nn.LayerNorm(g.shape[0], eps=cfg.eps)
        l.weight.data, l.bias.data = torch.from_numpy(g.copy()), torch.from_numpy(b.copy())
        return l

    def emb(t):
        e = nn.Embedding(*t.shape)
        e.weight.data = torch.from_numpy(t.copy())
        return e

    class Layer(nn.Module):
        def __init__(self, lw):
            super().__init__()
            self.q, self.k, self.v, self.o = lin(lw["wq"], lw["bq"]), lin(lw["wk"], lw["bk"]), lin(lw["wv"], lw["bv"]), lin(lw["wo"], lw["bo"])
            self.ln1, self.ln2 = ln(lw["ln1_g"], lw["ln1_b"]), ln(lw["ln2_g"], lw["ln2_b"])
            self.f1, self.f2, self.act = lin(lw["w1"], lw["b1"]), lin(lw["w2"], lw["b2"]), nn.GELU()

        def forward(self, x, mask):
            B, S, H = x.shape
            d = H // cfg.heads

            def heads(t):
                return t.view(B, S, cfg.heads, d).permute(0, 2, 1, 3)
            scores = torch.matmul(heads(self.q(x)), heads(self.k(x)).transpose(-1, -2)) / math.sqrt(d) + mask
            ctx = torch.matmul(torch.softmax(scores, -1), heads(self.v(x))).permute(0, 2, 1, 3).reshape(B, S, H)
            x = self.ln1(self.o(ctx) + x)
            return self.ln2(self.f2(self.act(self.f1(x))) + x)

    class Encoder(nn.Module):
        def __init__(self):
            super().__init__()
            self.word, self.ttype, self.pos = emb(w["word"]), emb(w["type"]), emb(w["pos"])
            self.ln = ln(w["emb_ln_g"], w["emb_ln_b"])
            self.layers = nn.ModuleList([Layer(lw) for lw in w["layers"]])
            self.register_buffer("position_ids", torch.arange(cfg.max_pos if dynamic_seq else seq).unsqueeze(0))

        def forward(self, input_ids, attention_mask, token_type_ids):
            pos = self.position_ids[:, :input_ids.shape[1]] if dynamic_seq else self.position_ids
            x = self.ln((self.word(input_ids) + self.ttype(token_type_ids)) + self.pos(pos))
            mask = (1.0 - attention_mask[:, None, None, :].to(torch.float32)) * torch.finfo(torch.float32).min
            for l in self.layers:
                x = l(x, mask)
            return x

    return Encoder().eval()


def encoder_onnx(cfg, w, batch, seq) -> bytes:
    import torch
    ids = torch.zeros(batch, seq, dtype=torch.int64)
    return export_bytes(encoder_module(cfg, w, seq), (ids, torch.ones_like(ids), torch.zeros_like(ids)),
                        ["input_ids", "attention_mask", "token_type_ids"], ["last_hidden_state"])


def embedding_head_config():
    """bert_module's sizes scaled down: 2 layers, hidden 32, 2 heads."""
    from rten_amd.workloads import bert as Bw
    return Bw.BertConfig(hidden=32, heads=2, layers=2, ffn=64, vocab=50, max_pos=16, type_vocab=2)


def embedding_head_module(cfg=None, w=None, seq: int = 5, p: float = 2.0, dynamic_seq: bool = False):
    """A sentence-embedding model: the encoder above, masked mean pooling over the tokens and F.normalize(p, dim=1).  The exporter writes the head as
    Unsqueeze / Cast / Mul / ReduceSum / Clip / Div for the pooling and ReduceL2 (p = 2) or ReduceL1 (p = 1) / Clip / Shape / Expand / Div for the
    normalisation."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as Fn
    from rten_amd.workloads import bert as Bw
    cfg = cfg if cfg is not None else embedding_head_config()
    w = w if w is not None else Bw.make_weights(cfg)

    class Head(nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder = encoder_module(cfg, w, seq, dynamic_seq)

        def forward(self, input_ids, attention_mask, token_type_ids):
            h = self.encoder(input_ids, attention_mask, token_type_ids)
            m = attention_mask.unsqueeze(-1).to(torch.float32)
            pooled = (h * m).sum(1) / torch.clamp(m.sum(1), min=1e-9)
            return Fn.normalize(pooled, p=p, dim=1)

    return Head().eval()


def embedding_head_onnx(model=None, batch: int = 2, seq: int = 5, dynamic: bool = False, p: float = 2.0) -> bytes:
    import torch
    model = model if model is not None else embedding_head_module(seq=seq, p=p, dynamic_seq=dynamic)
    ids = torch.zeros(batch, seq, dtype=torch.int64)
    names = ["input_ids", "attention_mask", "token_type_ids"]
    axes = dict({n: {0: "batch", 1: "seq"} for n in names}, embedding={0: "batch"}) if dynamic else None
    return export_bytes(model, (ids, torch.ones_like(ids), torch.zeros_like(ids)), names, ["embedding"], axes)


def reduce_zoo_module():
    """The reductions PyTorch's exporter writes as Reduce* nodes of their own: F.normalize(p=1) (ReduceL1), torch.logsumexp (ReduceLogSumExp),
    torch.linalg.vector_norm over two axes (ReduceL2), torch.prod (ReduceProd), and (x * x).sum, which it writes as Mul + ReduceSum -- the same value
    as a ReduceSumSquare only where the fused multiply-add rounds like the product and the add (the hand-built graph of rten_amd/onnx_writer.py has
    the ReduceSumSquare node)."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as Fn

    class Zoo(nn.Module):
        def forward(self, x):  # [N, 3, 4, 6]
            return (Fn.normalize(x, p=1.0, dim=-1), torch.logsumexp(x, dim=2), torch.linalg.vector_norm(x, dim=(1, 2)), torch.prod(x, dim=1), (x * x).sum(-1))

    return Zoo().eval()


ZOO_OUTPUTS = ["l1_normalized", "logsumexp", "norm2", "prod", "sum_of_squares"]


def reduce_zoo_onnx(model=None, batch: int = 2, dynamic: bool = True) -> bytes:
    import torch
    model = model if model is not None else reduce_zoo_module()
    axes = dict({"x": {0: "batch"}}, **{n: {0: "batch"} for n in ZOO_OUTPUTS}) if dynamic else None
    return export_bytes(model, (torch.zeros(batch, 3, 4, 6),), ["x"], ZOO_OUTPUTS, axes)


def bert_module(layers=2, hidden=768, heads=12, ffn=3072, vocab=30522, seed=0):
    import torch
    from transformers import BertConfig, BertModel
    torch.manual_seed(seed)
    cfg = BertConfig(vocab_size=vocab, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=ffn,
                     max_position_embeddings=512, hidden_act="gelu", attn_implementation="eager")
    return BertModel(cfg, add_pooling_layer=False).eval()


def bert_onnx(model, batch=2, seq=128) -> bytes:
    import torch
    ids = torch.zeros(batch, seq, dtype=torch.int64)
    return export_bytes(model, (ids, torch.ones_like(ids), torch.zeros_like(ids)), ["input_ids", "attention_mask", "token_type_ids"],
                        ["last_hidden_state"])


def mobile_module(width: int = 1, seed: int = 0):
    """A small MobileNetV2 / V3 / EfficientNet-style network whose exported graph holds every activation the backend runs:
    ReLU6 (Clip with min / max attributes), Hardswish, a Hardsigmoid squeeze-excite gate, SiLU (Sigmoid + Mul), a Sigmoid
    squeeze-excite gate, QuickGELU x * sigmoid(1.702 x) (Swish), LeakyReLU and ELU.  The squeezes are AdaptiveAvgPool2d(1)
    (GlobalAveragePool).  `width` scales the channel counts."""
    import torch
    from torch import nn
    torch.manual_seed(seed)
    c1, c2, c3 = 16 * width, 24 * width, 32 * width

    class SE(nn.Module):
        def __init__(self, c, r, inner, gate):
            super().__init__()
            self.pool, self.fc1, self.act, self.fc2, self.gate = nn.AdaptiveAvgPool2d(1), nn.Conv2d(c, r, 1), inner, nn.Conv2d(r, c, 1), gate

        def forward(self, x):
            return x * self.gate(self.fc2(self.act(self.fc1(self.pool(x)))))

    class QuickGelu(nn.Module):
        def forward(self, x):
            return x * torch.sigmoid(1.702 * x)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.body = nn.Sequential(
                nn.Conv2d(3, c1, 3, 2, 1), nn.ReLU6(),                               # stem, MobileNetV2
                nn.Conv2d(c1, c1, 3, 1, 1, groups=c1), nn.Hardswish(),               # depthwise, MobileNetV3
                SE(c1, 8, nn.ReLU(), nn.Hardsigmoid()),
                nn.Conv2d(c1, c2, 1), nn.SiLU(),                                     # pointwise, EfficientNet
                nn.Conv2d(c2, c2, 3, 2, 1, groups=c2), nn.SiLU(),
                SE(c2, 8, nn.SiLU(), nn.Sigmoid()),
                nn.Conv2d(c2, c3, 1), nn.LeakyReLU(0.1),
                nn.Conv2d(c3, c3, 3, 1, 1), nn.ELU(),
                QuickGelu(),
                nn.Conv2d(c3, c3, 1), nn.ReLU6(),
                nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(c3, 10))
            for m in self.modules():  # small weights: activations stay in the interesting range of every function
                if isinstance(m, nn.Conv2d):
                    nn.init.normal_(m.weight, 0.0, 0.7 / (m.weight[0].numel() ** 0.5))

        def forward(self, x):
            return self.body(x)

    return Net().eval()


def mobile_onnx(model=None, image: int = 32) -> bytes:
    import torch
    model = model if model is not None else mobile_module()
    return export_bytes(model, (torch.zeros(2, 3, image, image),), ["x"], ["logits"], {"x": {0: "batch"}, "logits": {0: "batch"}})


def yolo_module(seed: int = 0, reg_max: int = 8, classes: int = 4):
    """A small YOLOv8-style detector (the Ultralytics layout with BatchNorm folded): Conv + SiLU blocks, C2f blocks (a channel Split, a
    bottleneck, Concat), SPPF (three 5x5 stride-1 max-pools), a top-down path of two nearest 2x upsamplings each followed by a Concat, and a DFL
    box head (Reshape, Transpose, Softmax over axis 1, a 1x1 Conv whose weights are the bin indices) beside a Sigmoid class head.  The channel
    splits are torch.split with constant sizes (`chunk` does not export through export_bytes)."""
    import torch
    from torch import nn
    torch.manual_seed(seed)

    class Conv(nn.Module):
        def __init__(self, ci, co, k=1, s=1):
            super().__init__()
            self.conv, self.act = nn.Conv2d(ci, co, k, s, k // 2), nn.SiLU()

        def forward(self, x):
            return self.act(self.conv(x))

    class Bottleneck(nn.Module):
        def __init__(self, c, shortcut):
            super().__init__()
            self.cv1, self.cv2, self.add = Conv(c, c, 3), Conv(c, c, 3), shortcut

        def forward(self, x):
            y = self.cv2(self.cv1(x))
            return x + y if self.add else y

    class C2f(nn.Module):
        def __init__(self, ci, co, shortcut=True):
            super().__init__()
            self.c = co // 2
            self.cv1, self.cv2, self.m = Conv(ci, 2 * self.c), Conv(3 * self.c, co), Bottleneck(self.c, shortcut)

        def forward(self, x):
            a, b = torch.split(self.cv1(x), [self.c, self.c], 1)
            return self.cv2(torch.cat([a, b, self.m(b)], 1))

    class SPPF(nn.Module):
        def __init__(self, ci, co):
            super().__init__()
            self.cv1, self.cv2, self.pool = Conv(ci, ci // 2), Conv(ci // 2 * 4, co), nn.MaxPool2d(5, 1, 2)

        def forward(self, x):
            x = self.cv1(x)
            y1 = self.pool(x)
            y2 = self.pool(y1)
            return self.cv2(torch.cat([x, y1, y2, self.pool(y2)], 1))

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.stem, self.d1, self.d2 = Conv(3, 8, 3, 2), Conv(8, 16, 3, 2), Conv(16, 32, 3, 2)
            self.c2f1, self.d3, self.sppf = C2f(32, 32), Conv(32, 64, 3, 2), SPPF(64, 64)
            self.up = nn.Upsample(scale_factor=2, mode="nearest")
            self.c2f2, self.c2f3 = C2f(64 + 32, 32, False), C2f(32 + 16, 16, False)
            self.box, self.cls = nn.Conv2d(16, 4 * reg_max, 1), nn.Conv2d(16, classes, 1)
            self.dfl = nn.Conv2d(reg_max, 1, 1, bias=False)
            for m in self.modules():  # small weights: activations stay in the interesting range of SiLU / Softmax
                if isinstance(m, nn.Conv2d):
                    nn.init.normal_(m.weight, 0.0, 1.0 / (m.weight[0].numel() ** 0.5))
            self.dfl.weight.data[:] = torch.arange(reg_max, dtype=torch.float32).view(1, reg_max, 1, 1)

        def forward(self, x):
            p3 = self.d1(self.stem(x))   # stride 4
            p4 = self.c2f1(self.d2(p3))  # stride 8
            p5 = self.sppf(self.d3(p4))  # stride 16
            h4 = self.c2f2(torch.cat([self.up(p5), p4], 1))
            h3 = self.c2f3(torch.cat([self.up(h4), p3], 1))
            b, _, hh, ww = h3.shape
            box = self.box(h3).view(b, 4, reg_max, hh * ww).transpose(2, 1).softmax(1)  # DFL: [b, bins, 4, anchors]
            box = self.dfl(box).view(b, 4, hh * ww)
            return torch.cat([box, self.cls(h3).view(b, classes, hh * ww).sigmoid()], 1)

    return Net().eval()


def yolo_onnx(model=None, image: int = 64) -> bytes:
    import torch
    model = model if model is not None else yolo_module()
    return export_bytes(model, (torch.zeros(2, 3, image, image),), ["x"], ["y"], {"x": {0: "batch"}, "y": {0: "batch"}})


def classifier_topk_module(seed: int = 0):
    """The mobile network as an ImageNet-style classifier that finishes in the graph: softmax(-1), then topk(5).  Outputs: the probabilities (the
    pre-selection tensor), the five values and their indices."""
    import torch
    from torch import nn
    body = mobile_module(seed=seed)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.body = body

        def forward(self, x):
            probs = self.body(x).softmax(-1)
            values, indices = torch.topk(probs, 5)
            return probs, values, indices

    return Net().eval()


def classifier_topk_onnx(model=None, image: int = 32) -> bytes:
    import torch
    model = model if model is not None else classifier_topk_module()
    names = ["probs", "values", "indices"]
    return export_bytes(model, (torch.zeros(2, 3, image, image),), ["x"], names, {n: {0: "batch"} for n in ["x"] + names})


def segment_argmax_module(seed: int = 0, classes: int = 21):
    """A DeepLab-style segmentation head on the mobile network's features: a 1x1 class convolution at stride 4, bilinear interpolation back to the
    input size, argmax over the (strided) channel axis.  Outputs: the class map [b, classes, h, w] (the pre-selection tensor) and the labels [b, h, w]."""
    import torch
    from torch import nn
    import torch.nn.functional as F
    features = mobile_module(seed=seed).body[:8]  # through the second squeeze-excite block: 24 channels at stride 4
    torch.manual_seed(seed + 1)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.features, self.head = features, nn.Conv2d(24, classes, 1)

        def forward(self, x):
            logits = F.interpolate(self.head(self.features(x)), size=x.shape[2:], mode="bilinear", align_corners=False)
            return logits, logits.argmax(1)

    return Net().eval()


def segment_argmax_onnx(model=None, image: int = 32) -> bytes:
    import torch
    model = model if model is not None else segment_argmax_module()
    names = ["logits", "labels"]
    return export_bytes(model, (torch.zeros(2, 3, image, image),), ["x"], names, {n: {0: "batch"} for n in ["x"] + names})


def yolo_filter_module(seed: int = 0, keep: int = 20, classes: int = 4, batch: int = 2):
    """The YOLO-style detector with the usual score filter in the graph: the best class score of every anchor (`scores.max(1)`: ReduceMax + ArgMax), the
    `keep` best anchors (TopK over the anchor axis), and their boxes / classes fetched by the returned indices (per image `index_select`: Gather along the
    anchor axis).  Outputs: the detector's own [b, 4 + classes, anchors] tensor (pre-selection), the per-anchor confidence, the kept scores, their anchor
    indices, the kept boxes [b, 4, keep] and classes [b, keep].  The batch is static (the gathers are per image)."""
    import torch
    from torch import nn
    body = yolo_module(seed=seed, classes=classes)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.body = body

        def forward(self, x):
            y = self.body(x)
            conf, cls = y[:, 4:, :].max(1)
            top, idx = conf.topk(keep, dim=1)
            boxes = torch.stack([torch.index_select(y[i, :4, :], 1, idx[i]) for i in range(batch)], 0)
            kept_cls = torch.stack([torch.index_select(cls[i], 0, idx[i]) for i in range(batch)], 0)
            return y, conf, top, idx, boxes, kept_cls

    return Net().eval()


def yolo_filter_onnx(model=None, image: int = 64, batch: int = 2) -> bytes:
    import torch
    model = model if model is not None else yolo_filter_module(batch=batch)
    return export_bytes(model, (torch.zeros(batch, 3, image, image),), ["x"], ["y", "conf", "top", "idx", "boxes", "classes"])


def recognizer_module(kind: str = "gru", bidirectional: bool = True, layers: int = 1, seed: int = 0, height: int = 8, channels: int = 4, hidden: int = 20,
                      classes: int = 11, batch_first: bool = False, log_softmax: bool = False):
    """A text recogniser in the shape of `ocrs`: Conv2d + ReLU over a [b, 1, height, w] line image, every image column a time step
    (`permute(3, 0, 1, 2).flatten(2)` -> [w, b, channels * height]), `layers` uni- or bidirectional nn.GRU / nn.LSTM layers, a Linear head over
    the classes -- [w, b, classes], or [b, w, classes] with `batch_first` (a trailing permute: what the model ABI's dim-0 batch slices need).  The exporter writes one GRU / LSTM node per layer (linear_before_reset=1, empty sequence_lens, initial states from Expand /
    ConstantOfShape) between Transpose / Reshape / Shape arithmetic.  `log_softmax`: the model's real head, log_softmax(dim=-1) over the classes (what a
    CTC decoder reads): one LogSoftmax node."""
    import torch
    from torch import nn
    torch.manual_seed(seed)
    rnn_cls = {"gru": nn.GRU, "lstm": nn.LSTM}[kind]

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = nn.Conv2d(1, channels, 3, padding=1)
            self.rnn = rnn_cls(channels * height, hidden, num_layers=layers, bidirectional=bidirectional)
            self.head = nn.Linear(hidden * (2 if bidirectional else 1), classes)

        def forward(self, x):
            f = torch.relu(self.conv(x)).permute(3, 0, 1, 2).flatten(2)
            y, _ = self.rnn(f)
            y = self.head(y)
            if log_softmax:
                y = torch.log_softmax(y, dim=-1)
            return y.permute(1, 0, 2) if batch_first else y

    net = Net().eval()
    net.batch_first = batch_first  # (recognizer_onnx names the dynamic output axes by it)
    return net


def recognizer_onnx(model=None, kind: str = "gru", bidirectional: bool = True, layers: int = 1, seed: int = 0, batch: int = 2, width: int = 12,
                    height: int = 8, dynamic: bool = True) -> bytes:
    import torch
    model = model if model is not None else recognizer_module(kind, bidirectional, layers, seed, height=height)
    y_axes = {0: "batch", 1: "width"} if getattr(model, "batch_first", False) else {0: "width", 1: "batch"}
    axes = {"x": {0: "batch", 3: "width"}, "y": y_axes} if dynamic else None
    return export_bytes(model, (torch.zeros(batch, 1, height, width),), ["x"], ["y"], axes)


def generator_module(seed: int = 0, width: int = 8):
    """A small image-to-image generator in the shape of the CycleGAN / fast-style-transfer nets: Conv -> InstanceNorm2d(affine) -> ReLU down path (one
    stride-2 stage), two residual blocks with InstanceNorm, a ConvTranspose up path, Tanh.  Zero padding only (no Pad node).  Every
    nn.InstanceNorm2d exports as one InstanceNormalization node; those followed by a ReLU fuse with it in the executor."""
    import torch
    from torch import nn
    torch.manual_seed(seed)
    c1, c2 = width, 2 * width

    class Res(nn.Module):
        def __init__(self, c):
            super().__init__()
            self.body = nn.Sequential(nn.Conv2d(c, c, 3, 1, 1), nn.InstanceNorm2d(c, affine=True), nn.ReLU(), nn.Conv2d(c, c, 3, 1, 1), nn.InstanceNorm2d(c, affine=True))

        def forward(self, x):
            return x + self.body(x)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.body = nn.Sequential(
                nn.Conv2d(3, c1, 3, 1, 1), nn.InstanceNorm2d(c1, affine=True), nn.ReLU(),
                nn.Conv2d(c1, c2, 3, 2, 1), nn.InstanceNorm2d(c2, affine=True), nn.ReLU(),
                Res(c2), Res(c2),
                nn.ConvTranspose2d(c2, c1, 3, 2, 1, output_padding=1), nn.InstanceNorm2d(c1, affine=True), nn.ReLU(),
                nn.Conv2d(c1, 3, 3, 1, 1), nn.Tanh())
            for m in self.modules():  # distinct scale / bias per channel: a channel mix-up cannot cancel
                if isinstance(m, nn.InstanceNorm2d):
                    nn.init.uniform_(m.weight, 0.5, 1.5)
                    nn.init.uniform_(m.bias, -0.5, 0.5)

        def forward(self, x):
            return self.body(x)

    return Net().eval()


def generator_onnx(model=None, image: int = 16, batch: int = 2, dynamic: bool = True) -> bytes:
    import torch
    model = model if model is not None else generator_module()
    axes = {"x": {0: "batch"}, "y": {0: "batch"}} if dynamic else None
    return export_bytes(model, (torch.zeros(batch, 3, image, image),), ["x"], ["y"], axes)


def preact_module(seed: int = 0, classes: int = 5):
    """A pre-activation network (BN -> ReLU -> Conv, the order of ResNet-v2 / DenseNet) whose BatchNormalization nodes survive export: the exporter
    folds a BatchNorm only into a convolution directly before it.  Here one follows a convolution whose output is also the residual, one follows a
    pool (with a LeakyReLU), and a BatchNorm1d sits in the head in front of the Linear layer."""
    import torch
    from torch import nn
    torch.manual_seed(seed)

    def randomise(bn):  # running statistics and affine parameters away from their (0, 1, 1, 0) initial values
        nn.init.uniform_(bn.weight, 0.5, 1.5)
        nn.init.uniform_(bn.bias, -0.5, 0.5)
        bn.running_mean.uniform_(-0.5, 0.5)
        bn.running_var.uniform_(0.5, 2.0)
        return bn

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.stem = nn.Conv2d(3, 8, 3, 1, 1)
            self.bn1, self.conv1 = randomise(nn.BatchNorm2d(8)), nn.Conv2d(8, 8, 3, 1, 1)
            self.pool = nn.MaxPool2d(2)
            self.bn2, self.act2, self.conv2 = randomise(nn.BatchNorm2d(8)), nn.LeakyReLU(0.1), nn.Conv2d(8, 12, 1)
            self.bn3, self.fc = randomise(nn.BatchNorm1d(12)), nn.Linear(12, classes)

        def forward(self, x):
            y = self.stem(x)
            y = y + self.conv1(torch.relu(self.bn1(y)))
            y = self.conv2(self.act2(self.bn2(self.pool(y))))
            y = torch.flatten(nn.functional.adaptive_avg_pool2d(y, 1), 1)
            return self.fc(self.bn3(y))

    return Net().eval()


def preact_onnx(model=None, image: int = 16, batch: int = 2, dynamic: bool = True) -> bytes:
    import torch
    model = model if model is not None else preact_module()
    axes = {"x": {0: "batch"}, "logits": {0: "batch"}} if dynamic else None
    return export_bytes(model, (torch.zeros(batch, 3, image, image),), ["x"], ["logits"], axes)


def reflect_generator_module(seed: int = 0, width: int = 8):
    """The image-to-image generator as such nets are written: a ReflectionPad2d(3) + 7x7 stem, residual blocks of ReflectionPad2d(1) + 3x3 convolutions with
    InstanceNorm and nn.PReLU(c), a ReplicationPad2d in front of the output convolution, and one F.pad with a negative entry (a crop and a zero pad in one
    node).  Exports Pad nodes with mode reflect / edge / constant, and PRelu with a [C, 1, 1] slope."""
    import torch
    from torch import nn
    torch.manual_seed(seed)
    c = width

    class Res(nn.Module):
        def __init__(self, c):
            super().__init__()
            self.body = nn.Sequential(nn.ReflectionPad2d(1), nn.Conv2d(c, c, 3), nn.InstanceNorm2d(c, affine=True), nn.PReLU(c),
                                      nn.ReflectionPad2d(1), nn.Conv2d(c, c, 3), nn.InstanceNorm2d(c, affine=True))

        def forward(self, x):
            return x + self.body(x)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.stem = nn.Sequential(nn.ReflectionPad2d(3), nn.Conv2d(3, c, 7), nn.InstanceNorm2d(c, affine=True), nn.PReLU(c))
            self.blocks = nn.Sequential(Res(c), Res(c))
            self.out = nn.Sequential(nn.ReplicationPad2d(1), nn.Conv2d(c, 3, 3), nn.Tanh())
            for m in self.modules():
                if isinstance(m, nn.InstanceNorm2d):
                    nn.init.uniform_(m.weight, 0.5, 1.5)
                    nn.init.uniform_(m.bias, -0.5, 0.5)
                if isinstance(m, nn.PReLU):
                    nn.init.uniform_(m.weight, 0.05, 0.45)

        def forward(self, x):
            y = self.blocks(self.stem(x))
            y = nn.functional.pad(y, (1, -2, -1, 2))  # W: one zero column in front, two cropped at the end; H: one row cropped, two zero rows appended
            return self.out(y)

    return Net().eval()


def reflect_generator_onnx(model=None, image: int = 16, batch: int = 2, dynamic: bool = True) -> bytes:
    import torch
    model = model if model is not None else reflect_generator_module()
    axes = {"x": {0: "batch"}, "y": {0: "batch"}} if dynamic else None
    return export_bytes(model, (torch.zeros(batch, 3, image, image),), ["x"], ["y"], axes)


def gpt2_mlp_module(seed: int = 0, hidden: int = 32, ffn: int = 96):
    """A GPT-2 block's MLP half: LayerNorm, Linear, `gelu_new` written out (0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))) with torch.pow(x, 3.0)),
    Linear.  Exports Pow with a scalar exponent of 3 between Mul / Add / Tanh nodes."""
    import math
    import torch
    from torch import nn
    torch.manual_seed(seed)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.ln, self.fc, self.proj = nn.LayerNorm(hidden), nn.Linear(hidden, ffn), nn.Linear(ffn, hidden)
            nn.init.uniform_(self.ln.weight, 0.5, 1.5)
            nn.init.uniform_(self.ln.bias, -0.5, 0.5)

        def forward(self, x):
            h = self.fc(self.ln(x))
            h = 0.5 * h * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (h + 0.044715 * torch.pow(h, 3.0))))
            return self.proj(h)

    return Net().eval()


def gpt2_mlp_onnx(model=None, batch: int = 2, seq: int = 5, hidden: int = 32, dynamic: bool = True) -> bytes:
    import torch
    model = model if model is not None else gpt2_mlp_module(hidden=hidden)
    axes = {"x": {0: "batch"}, "y": {0: "batch"}} if dynamic else None
    return export_bytes(model, (torch.zeros(batch, seq, hidden),), ["x"], ["y"], axes)


BOX_IMAGE = (48.0, 64.0)  # (height, width) the box decoder clips against


def box_decode_module(seed: int = 0, anchors: int = 3):
    """A detection head's decode step: a 3x3 convolution gives (dx, dy, dw, dh) per anchor and cell; centres move by the offsets, sizes scale by exp(dw / dh),
    the corners are clipped to the image with torch.maximum / torch.minimum, and a few per-box statistics use sqrt, reciprocal, neg and abs.  Exports Exp,
    Min, Max, Sqrt, Reciprocal, Neg and Abs around Mul / Add / Sub / Div / Slice / Concat."""
    import torch
    from torch import nn
    torch.manual_seed(seed)
    a = anchors

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.head = nn.Conv2d(4, 4 * a, 3, 1, 1)
            self.register_buffer("anchor_wh", torch.rand(1, 2 * a, 1, 1) * 12 + 4)
            self.register_buffer("lo", torch.zeros(1, 1, 1, 1))
            self.register_buffer("hi_x", torch.full((1, 1, 1, 1), BOX_IMAGE[1]))
            self.register_buffer("hi_y", torch.full((1, 1, 1, 1), BOX_IMAGE[0]))

        def forward(self, x, grid):
            t = self.head(x)                                      # [N, 4a, H, W]
            cx = grid[:, 0:1] + t[:, 0:a]                         # centres: the cell's position plus the offsets
            cy = grid[:, 1:2] + t[:, a:2 * a]
            wh = torch.exp(t[:, 2 * a:]) * self.anchor_wh         # sizes
            w, h = wh[:, :a], wh[:, a:]
            x0 = torch.maximum(cx - w * 0.5, self.lo)
            y0 = torch.maximum(cy - h * 0.5, self.lo)
            x1 = torch.minimum(cx + w * 0.5, self.hi_x)
            y1 = torch.minimum(cy + h * 0.5, self.hi_y)
            side = torch.sqrt(torch.abs((x1 - x0) * (y1 - y0)))   # geometric mean side of the clipped box (Abs: a box clipped away has a negative extent)
            inv = torch.reciprocal(side + 1.0)
            return torch.cat([x0, y0, x1, y1, side, inv, torch.neg(torch.abs(t[:, 0:a]))], 1)

    return Net().eval()


def box_decode_onnx(model=None, batch: int = 2, height: int = 6, width: int = 8, dynamic: bool = True) -> bytes:
    import torch
    model = model if model is not None else box_decode_module()
    axes = {"x": {0: "batch"}, "boxes": {0: "batch"}} if dynamic else None
    return export_bytes(model, (torch.zeros(batch, 4, height, width), torch.zeros(1, 2, height, width)), ["x", "grid"], ["boxes"], axes)


def dynamic_upsample_weights(seed: int = 0):
    rng = np.random.default_rng(seed)
    return {"a.weight": rng.normal(0, 0.3, (4, 3, 3, 3)).astype(np.float32), "a.bias": rng.normal(0, 0.1, 4).astype(np.float32),
            "b.weight": rng.normal(0, 0.3, (3, 4, 3, 3)).astype(np.float32), "b.bias": rng.normal(0, 0.1, 3).astype(np.float32)}


def dynamic_upsample_onnx(weights=None, scale: float = 2.0) -> bytes:
    """Conv -> F.interpolate(scale_factor=scale, nearest) -> F.pad(1, value 0.5) -> Conv with dynamic N / H / W, in the form exporters give the output size under
    dynamic axes: Shape -> Slice -> Cast -> Mul -> Floor -> Cast -> Concat -> Resize(sizes).  This torch's TorchScript exporter passes `scales` to Resize
    instead (no shape arithmetic at all), so the graph is written with rten_amd/onnx_writer.py; the Pad takes its pads and constant_value as inputs (the
    opset 11+ form; the exporter's own Pad nodes carry attributes)."""
    from rten_amd import onnx_writer as ow
    w = weights if weights is not None else dynamic_upsample_weights()
    i64 = lambda *v: np.array(v, np.int64)
    inits = [ow.tensor(k, v) for k, v in w.items()] + [
        ow.tensor("c0", i64(0)), ow.tensor("c2", i64(2)), ow.tensor("c4", i64(4)), ow.tensor("scale", np.array([scale, scale], np.float32)),
        ow.tensor("pads", i64(0, 0, 1, 1, 0, 0, 1, 1)), ow.tensor("pad_value", np.array(0.5, np.float32))]
    nodes = [
        ow.node("Conv", ["x", "a.weight", "a.bias"], ["a"], name="conv_a", kernel_shape=[3, 3], pads=[1, 1, 1, 1]),
        ow.node("Shape", ["a"], ["shape"], name="shape"),
        ow.node("Slice", ["shape", "c0", "c2", "c0"], ["nc"], name="slice_nc"),
        ow.node("Slice", ["shape", "c2", "c4", "c0"], ["hw"], name="slice_hw"),
        ow.node("Cast", ["hw"], ["hw_f"], name="cast_f", to=1),
        ow.node("Mul", ["hw_f", "scale"], ["hw_scaled"], name="mul_scale"),
        ow.node("Floor", ["hw_scaled"], ["hw_floor"], name="floor_hw"),
        ow.node("Cast", ["hw_floor"], ["hw_i"], name="cast_i", to=7),
        ow.node("Concat", ["nc", "hw_i"], ["sizes"], name="concat_sizes", axis=0),
        ow.node("Resize", ["a", "", "", "sizes"], ["up"], name="resize", mode="nearest", coordinate_transformation_mode="asymmetric", nearest_mode="floor"),
        ow.node("Pad", ["up", "pads", "pad_value"], ["padded"], name="pad_up", mode="constant"),
        ow.node("Conv", ["padded", "b.weight", "b.bias"], ["y"], name="conv_b", kernel_shape=[3, 3], pads=[0, 0, 0, 0]),
    ]
    return ow.model(nodes, [ow.value_info("x", 1, ["batch", 3, "height", "width"])], [ow.value_info("y", 1, ["batch", 3, "height2", "width2"])], inits)


def warp_module(seed: int = 0, channels: int = 4, align_corners: bool = False):
    """Flow warping as video and stereo networks write it: a 3x3 convolution makes features, another predicts a two-channel flow from them, and
    F.grid_sample(bilinear, zeros) reads the features at the identity grid (an input, one per batch row: it has the image's size) plus the flow.  The exporter
    writes Conv / Conv / Tanh / Mul / Transpose / Add / GridSample(mode="bilinear", padding_mode="zeros", align_corners)."""
    import torch
    from torch import nn
    import torch.nn.functional as Fn
    torch.manual_seed(seed)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.feat = nn.Conv2d(3, channels, 3, 1, 1)
            self.flow = nn.Conv2d(channels, 2, 3, 1, 1)

        def forward(self, x, grid):
            f = self.feat(x)
            flow = torch.tanh(self.flow(f)) * 0.5                  # [N, 2, H, W], offsets of up to half the image either way (some samples fall outside)
            return Fn.grid_sample(f, grid + flow.permute(0, 2, 3, 1), mode="bilinear", padding_mode="zeros", align_corners=align_corners)

    return Net().eval()


def warp_onnx(model=None, batch: int = 2, height: int = 6, width: int = 8, dynamic: bool = True, align_corners: bool = False) -> bytes:
    """Inputs x [batch, 3, H, W] and grid [batch, H, W, 2] (rten_amd.onnx_writer.base_grid for every row), output warped [batch, channels, H, W]."""
    import torch
    model = model if model is not None else warp_module(align_corners=align_corners)
    axes = {"x": {0: "batch"}, "grid": {0: "batch"}, "warped": {0: "batch"}} if dynamic else None
    return export_bytes(model, (torch.zeros(batch, 3, height, width), torch.zeros(batch, height, width, 2)), ["x", "grid"], ["warped"], axes)


def pixel_shuffle_sr_onnx(weights, block: int = 2, batch: int = 2, height: int = 5, width: int = 7) -> bytes:
    """rten_amd.onnx_writer.subpixel_sr_graph's network (same weights dict) with nn.PixelShuffle for the DepthToSpace: the exporter writes it as
    Reshape / 6-D Transpose / Reshape, the same permutation as DepthToSpace(mode="CRD").  Static shapes (the Reshape targets are constants)."""
    import torch
    from torch import nn

    def conv(w, b):
        c = nn.Conv2d(w.shape[1], w.shape[0], 3, 1, 1)
        c.weight.data, c.bias.data = torch.from_numpy(w.copy()), torch.from_numpy(b.copy())
        return c
    net = nn.Sequential(conv(*weights["c1"]), nn.ReLU(), conv(*weights["c2"]), nn.PixelShuffle(block)).eval()
    return export_bytes(net, (torch.zeros(batch, 3, height, width),), ["x"], ["y"])


def roberta_module(layers: int = 1, hidden: int = 32, heads: int = 2, ffn: int = 64, vocab: int = 100, positions: int = 40, seed: int = 0):
    """transformers' RobertaModel (eager attention, no pooling layer), random init.  Beside what BertModel exports it holds one CumSum --
    create_position_ids_from_input_ids: cumsum(mask, dim=1) * mask + padding_idx on int32 data -- and one GatherElements, torch.gather(buffered
    token_type_ids, 1, position_ids)."""
    import torch
    from transformers import RobertaConfig, RobertaModel
    torch.manual_seed(seed)
    cfg = RobertaConfig(vocab_size=vocab, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=ffn,
                        max_position_embeddings=positions, hidden_act="gelu", attn_implementation="eager", pad_token_id=1, bos_token_id=0, eos_token_id=2)
    return RobertaModel(cfg, add_pooling_layer=False).eval()


def roberta_onnx(model=None, batch: int = 2, seq: int = 7, dynamic: bool = False) -> bytes:
    """Inputs input_ids and attention_mask [batch, seq] (int64), output last_hidden_state; `dynamic`: free batch and sequence axes."""
    import torch
    model = model if model is not None else roberta_module()
    ids = torch.full((batch, seq), 5, dtype=torch.int64)
    axes = {"input_ids": {0: "batch", 1: "seq"}, "attention_mask": {0: "batch", 1: "seq"}, "last_hidden_state": {0: "batch", 1: "seq"}} if dynamic else None
    return export_bytes(model, (ids, torch.ones_like(ids)), ["input_ids", "attention_mask"], ["last_hidden_state"], axes)


CAUSAL_DECODER_PAD = 1


def causal_decoder_module(seed: int = 0, vocab: int = 50, hidden: int = 16, heads: int = 2, positions: int = 40):
    """A small decoder block in plain torch.nn: token + position embeddings with positions from cumsum(ids.ne(pad).int(), 1) * mask + pad (CumSum on int32),
    one attention block whose scores get torch.triu(torch.full((S, S), -inf), diagonal=1) (Trilu), torch.gather(y, 1, last_token_index) picking each
    row's last non-pad token (GatherElements), and a .repeat(1, 3, 2) output (Tile).  forward(ids [B, S]) -> [B, 3, 2 * hidden]."""
    import torch
    from torch import nn
    torch.manual_seed(seed)
    pad = CAUSAL_DECODER_PAD

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.tok = nn.Embedding(vocab, hidden)
            self.pos = nn.Embedding(positions, hidden)
            self.qkv = nn.Linear(hidden, 3 * hidden)
            self.proj = nn.Linear(hidden, hidden)
            self.norm = nn.LayerNorm(hidden)

        def forward(self, ids):
            b, s = ids.shape[0], ids.shape[1]
            mask = ids.ne(pad).int()
            positions_ = (torch.cumsum(mask, dim=1) * mask).long() + pad
            x = self.tok(ids) + self.pos(positions_)
            q, k, v = self.qkv(x).view(b, s, 3, heads, hidden // heads).permute(2, 0, 3, 1, 4)
            scores = q @ k.transpose(-1, -2) * (float(hidden // heads) ** -0.5)
            scores = scores + torch.triu(torch.full((s, s), float("-inf")), diagonal=1)
            a = torch.softmax(scores, dim=-1) @ v                                             # [B, heads, S, hidden / heads]
            y = self.norm(x + self.proj(a.permute(0, 2, 1, 3).reshape(b, s, hidden)))
            last = (mask.float().sum(dim=1, keepdim=True) - 1).clamp(min=0).long()            # [B, 1]: each row's last non-pad token
            picked = torch.gather(y, 1, last.unsqueeze(-1).expand(b, 1, hidden))              # [B, 1, hidden]
            return picked.repeat(1, 3, 2)

    return Net().eval()


def causal_decoder_onnx(model=None, batch: int = 2, seq: int = 6, dynamic: bool = False) -> bytes:
    """Input ids [batch, seq] (int64), output y [batch, 3, 2 * hidden].  Static: the mask is a constant the exporter folds or a Trilu of a constant; `dynamic`
    (free batch / sequence): the Trilu operand and the Tile repeats are run-time shape arithmetic."""
    import torch
    model = model if model is not None else causal_decoder_module()
    ids = torch.full((batch, seq), 5, dtype=torch.int64)
    axes = {"ids": {0: "batch", 1: "seq"}, "y": {0: "batch"}} if dynamic else None
    return export_bytes(model, (ids,), ["ids"], ["y"], axes)


if __name__ == "__main__":
    kind, path = sys.argv[1], sys.argv[2]
    if kind == "resnet50":
        from rten_amd.workloads import resnet50 as R
        data = resnet50_onnx(R.make_weights())
    elif kind == "encoder":  # BERT-base sized (BASELINE configs[3]): 12 layers, hidden 768, 12 heads, batch 32 x 128 tokens
        from rten_amd.workloads import bert as Bw
        cfg = Bw.BertConfig()
        data = encoder_onnx(cfg, Bw.make_weights(cfg), 32, 128)
    elif kind == "mobile":
        data = mobile_onnx()
    elif kind == "yolo":
        data = yolo_onnx()
    elif kind == "classifier_topk":
        data = classifier_topk_onnx()
    elif kind == "segment_argmax":
        data = segment_argmax_onnx()
    elif kind == "yolo_filter":
        data = yolo_filter_onnx()
    elif kind in ("recognizer_gru", "recognizer_lstm"):
        data = recognizer_onnx(kind=kind.split("_")[1])
    elif kind == "recognizer_ctc":
        data = recognizer_onnx(recognizer_module("gru", log_softmax=True))
    elif kind == "generator":
        data = generator_onnx()
    elif kind == "preact":
        data = preact_onnx()
    elif kind == "reflect_generator":
        data = reflect_generator_onnx()
    elif kind == "gpt2_mlp":
        data = gpt2_mlp_onnx()
    elif kind == "box_decode":
        data = box_decode_onnx()
    elif kind == "dynamic_upsample":
        data = dynamic_upsample_onnx()
    elif kind == "embedding_head":
        data = embedding_head_onnx(dynamic=True)
    elif kind == "reduce_zoo":
        data = reduce_zoo_onnx()
    elif kind == "roberta":
        data = roberta_onnx(dynamic=True)
    elif kind == "causal_decoder":
        data = causal_decoder_onnx(dynamic=True)
    elif kind == "warp":
        data = warp_onnx()
    elif kind == "pixel_shuffle_sr":
        from rten_amd import onnx_writer as ow
        data = pixel_shuffle_sr_onnx(ow.subpixel_sr_graph("CRD")[1])
    else:
        data = bert_onnx(bert_module())
    open(path, "wb").write(data)
    print(f"wrote {path}: {len(data)} bytes")


def log_mel_module(n_fft: int = 400, hop: int = 160, n_mels: int = 80):
    """The log-mel front end of a Whisper-style model: torch.stft(center=True, reflect) -> re^2 + im^2 -> mel MatMul -> clamp -> log10 -> maximum(l, l.max() - 8)
    -> (l + 4) / 4, with onnx_writer's Hann window and mel filterbank.  wave [batch, samples] -> [batch, frames, n_mels].  -> (module, {"window", "mel"})."""
    import torch
    from rten_amd import onnx_writer as ow
    w = {"window": ow.hann_window(n_fft), "mel": ow.mel_filterbank(n_fft, n_mels)}

    class LogMel(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.register_buffer("window", torch.from_numpy(w["window"]))
            self.register_buffer("mel", torch.from_numpy(w["mel"]))

        def forward(self, wave):
            s = torch.stft(wave, n_fft, hop, window=self.window, center=True, pad_mode="reflect", return_complex=False)
            power = s[..., 0] ** 2 + s[..., 1] ** 2
            l = torch.clamp(power.transpose(1, 2) @ self.mel, min=1e-10).log10()
            l = torch.maximum(l, l.max() - 8.0)
            return (l + 4.0) / 4.0

    return LogMel(), w


def log_mel_onnx(n_fft: int = 400, hop: int = 160, n_mels: int = 80, batch: int = 2, samples: int = 2000):
    """log_mel_module through PyTorch's exporter at opset 17, input `wave` [batch, samples] (both dynamic), output `log_mel`.  -> (model bytes, weights)."""
    import torch
    model, w = log_mel_module(n_fft, hop, n_mels)
    wave = torch.zeros(batch, samples)
    return export_bytes(model, (wave,), ["wave"], ["log_mel"], {"wave": {0: "batch", 1: "samples"}, "log_mel": {0: "batch", 1: "frames"}}, opset=17), w
