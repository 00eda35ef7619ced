// C ABI: ONNX graph slots.
#include "capi_internal.h"

GraphSlot& graph_slot(fe_ctx* ctx, int slot) {
  FE_CHECK(slot >= 0 && slot < FE_GRAPH_SLOTS, "graph slot %d out of range", slot);
  FE_CHECK(ctx->c.graphs[slot], "no graph loaded in slot %d", slot);
  return *ctx->c.graphs[slot];
}

extern "C" {

int fe_onnx_probe(const void* onnx_bytes, size_t len, int* n_nodes, int* n_initializers, int* n_outputs, int64_t in_dims[4],
                  char* err, int err_cap) {
  try {
    onnx::Model m;
    onnx::parse_model((const uint8_t*)onnx_bytes, len, m);
    if (n_nodes) *n_nodes = (int)m.nodes.size();
    if (n_initializers) *n_initializers = (int)m.init.size();
    if (n_outputs) *n_outputs = (int)m.outputs.size();
    if (in_dims)
      for (int k = 0; k < 4; ++k) in_dims[k] = k < (int)m.inputs[0].dims.size() ? m.inputs[0].dims[k] : -1;
  } catch (const std::exception& e) {
    if (err && err_cap > 0) snprintf(err, err_cap, "%s", e.what());
    return FE_ERR_RUNTIME;
  }
  return FE_OK;
}
int fe_graph_load(fe_ctx* ctx, int slot, const void* onnx_bytes, size_t len) {
  return fe_api(ctx, [&] {
    FE_CHECK(slot >= 0 && slot < FE_GRAPH_SLOTS && onnx_bytes && len > 0, "bad arguments");
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    FE_HIP(hipStreamSynchronize(ctx->c.stream));
    auto gs = std::make_unique<GraphSlot>();
    gs->g.load((const uint8_t*)onnx_bytes, len);
    ctx->c.graphs[slot] = std::move(gs);
  });
}
int fe_graph_unload(fe_ctx* ctx, int slot) {
  return fe_api(ctx, [&] {
    FE_CHECK(slot >= 0 && slot < FE_GRAPH_SLOTS, "bad arguments");
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    FE_HIP(hipStreamSynchronize(ctx->c.stream));
    ctx->c.graphs[slot].reset();
  });
}
int fe_graph_loaded(fe_ctx* ctx, int slot) {
  return ctx && slot >= 0 && slot < FE_GRAPH_SLOTS && ctx->c.graphs[slot] != nullptr;
}
int fe_graph_info(fe_ctx* ctx, int slot, int* n_nodes, int* n_outputs, int64_t in_dims[4], int* flags) {
  return fe_api(ctx, [&] {
    GraphSlot& gs = graph_slot(ctx, slot);
    const auto& m = gs.g.model();
    if (n_nodes) *n_nodes = (int)m.nodes.size();
    if (n_outputs) *n_outputs = (int)m.outputs.size();
    if (in_dims)
      for (int k = 0; k < 4; ++k) in_dims[k] = k < (int)m.inputs[0].dims.size() ? m.inputs[0].dims[k] : -1;
    if (flags) *flags = (gs.g.head_has_sub() ? 1 : 0) | (gs.g.head_has_mul() ? 2 : 0);
  });
}

int fe_graph_run(fe_ctx* ctx, int slot, const float* x, int n, int c, int h, int w, int on_device) {
  return fe_api(ctx, [&] {
    Ctx& C = ctx->c;
    GraphSlot& gs = graph_slot(ctx, slot);
    FE_CHECK(x && n > 0 && c > 0 && h > 0 && w > 0, "bad arguments");
    C.arena.reset();
    const int cp = Graph::pad_channels(c);
    Tensor xt;
    if (on_device) {
      xt = C.arena.tensor(n, h, w, cp);
      launch_nchw_to_nhwc(x, xt.p, n, c, h, w, cp, C.stream);
    } else {
      xt = upload_nchw(C, x, n, c, h, w, cp);
    }
    std::vector<GraphOutput> outs;
    gs.g.run(C, xt, c, outs);
    gs.last.clear();
    for (auto& o : outs) {
      GraphSlot::Out h_out;
      h_out.name = o.name; h_out.dims = o.dims;
      h_out.data.resize(o.numel);
      if (o.numel) FE_HIP(hipMemcpyAsync(h_out.data.data(), o.dev, o.numel * sizeof(float), hipMemcpyDeviceToHost, C.stream));
      gs.last.push_back(std::move(h_out));
    }
    FE_HIP(hipStreamSynchronize(C.stream));
  });
}
int fe_graph_output_info(fe_ctx* ctx, int slot, int i, char* name, int name_cap, int64_t dims[6], int* rank) {
  return fe_api(ctx, [&] {
    GraphSlot& gs = graph_slot(ctx, slot);
    FE_CHECK(i >= 0 && i < (int)gs.last.size(), "output index %d out of range (%zu outputs)", i, gs.last.size());
    const auto& o = gs.last[i];
    FE_CHECK(o.dims.size() <= 6, "output rank %zu", o.dims.size());
    if (name && name_cap > 0) snprintf(name, name_cap, "%s", o.name.c_str());
    if (rank) *rank = (int)o.dims.size();
    if (dims) for (size_t k = 0; k < o.dims.size(); ++k) dims[k] = o.dims[k];
  });
}
int fe_graph_output_copy(fe_ctx* ctx, int slot, int i, float* dst, size_t cap_floats) {
  return fe_api(ctx, [&] {
    GraphSlot& gs = graph_slot(ctx, slot);
    FE_CHECK(i >= 0 && i < (int)gs.last.size() && dst, "bad arguments");
    FE_CHECK(cap_floats >= gs.last[i].data.size(), "destination holds %zu floats, output has %zu", cap_floats, gs.last[i].data.size());
    if (!gs.last[i].data.empty()) memcpy(dst, gs.last[i].data.data(), gs.last[i].data.size() * sizeof(float));
  });
}

}  // extern "C"
