// Python bindings for the esr_amd gfx950 HIP extension.
#include <torch/extension.h>

// deform_conv.hip
at::Tensor deform_conv2d_forward(
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const c10::optional<at::Tensor>&,
    int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t);
std::vector<at::Tensor> deform_conv2d_backward(
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&,
    int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t);
std::vector<at::Tensor> deform_conv2d_forward_cols(
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const c10::optional<at::Tensor>&,
    int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t);
std::vector<at::Tensor> deform_conv2d_backward_cols(
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const c10::optional<at::Tensor>&,
    int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
    const std::string&);
at::Tensor deform_conv2d_forward_fused(
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const c10::optional<at::Tensor>&, int64_t);
at::Tensor deform_im2col_debug(
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
    int64_t);

// gru_gates.hip
std::vector<at::Tensor> gru_gates_ur_forward(const at::Tensor&,
                                             const at::Tensor&);
std::vector<at::Tensor> gru_gates_ur_backward(
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const at::Tensor&, const at::Tensor&);
std::vector<at::Tensor> gru_gates_out_forward(const at::Tensor&,
                                              const at::Tensor&,
                                              const at::Tensor&);
std::vector<at::Tensor> gru_gates_out_backward(
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&);

// event_ops.hip
at::Tensor splat_count(const at::Tensor&, int64_t, int64_t);
at::Tensor splat_stack(const at::Tensor&, int64_t, int64_t, int64_t, double,
                       double);
int64_t grid_cap();

// conv2d.hip
at::Tensor conv2d_fwd_mfma(const at::Tensor&, const at::Tensor&,
                           const c10::optional<at::Tensor>&,
                           int64_t, int64_t, int64_t, int64_t);
at::Tensor conv2d_fwd_valu(const at::Tensor&, const at::Tensor&,
                           const c10::optional<at::Tensor>&, int64_t, int64_t);
at::Tensor conv2d_fwd_valu2(const at::Tensor&, const at::Tensor&,
                            const c10::optional<at::Tensor>&, int64_t, int64_t);
at::Tensor conv2d_dgrad_s2(const at::Tensor&, const at::Tensor&,
                           int64_t, int64_t);
at::Tensor conv2d_wgrad_mfma(const at::Tensor&, const at::Tensor&,
                             int64_t, int64_t, int64_t, int64_t);
at::Tensor conv2d_s1(const at::Tensor&, const at::Tensor&,
                     const c10::optional<at::Tensor>&, int64_t, bool);
at::Tensor conv2d_wgrad_s1(const at::Tensor&, const at::Tensor&, int64_t);
at::Tensor act_grad(const at::Tensor&, const at::Tensor&, int64_t);
std::vector<at::Tensor> act_grad_bias(const at::Tensor&, const at::Tensor&,
                                      int64_t, bool);
std::vector<at::Tensor> bias_grad(const at::Tensor&, bool);
int64_t bias_grad_chain(int64_t, int64_t, int64_t);
int64_t bias_grad_chunk();
at::Tensor gemm16_probe(const at::Tensor&, const at::Tensor&);

// redistribute.hip
std::vector<at::Tensor> redistribute_stack_hip(const at::Tensor&, int64_t,
                                               int64_t, int64_t, int64_t);

// flat_adam.hip
void flat_grad_finite_check(const at::Tensor&, at::Tensor&);
void flat_adam_step(at::Tensor&, const at::Tensor&, at::Tensor&, at::Tensor&,
                    const c10::optional<at::Tensor>&, const at::Tensor&,
                    double, double, double, double, bool);
void flat_scale_update(at::Tensor&, bool, double, double, int64_t, double,
                       double);
void flat_grad_stats(const at::Tensor&, at::Tensor&, at::Tensor&, at::Tensor&,
                     double);
void flat_adam_step_clipped(at::Tensor&, const at::Tensor&, at::Tensor&,
                            at::Tensor&, const c10::optional<at::Tensor>&,
                            const at::Tensor&, const at::Tensor&, double,
                            double, double, double, bool);

// stream_ingest.hip
void stream_window_advance(at::Tensor&, const at::Tensor&);
void stream_splat_ragged(const at::Tensor&, const at::Tensor&,
                         const at::Tensor&, at::Tensor&, int64_t);

// batch_splat.hip
void evs_batch_splat(const at::Tensor&, const at::Tensor&, at::Tensor&,
                     int64_t, int64_t, int64_t);
int64_t evs_batch_splat_chunk();

// eval_metrics.hip
at::Tensor restoration_metrics(const at::Tensor&, const at::Tensor&, double);
std::vector<int64_t> restoration_metrics_tile();

// sr_emit.hip
std::vector<at::Tensor> sr_emit_scratch(const at::Tensor&, int64_t, int64_t);
at::Tensor sr_emit_counts(const at::Tensor&, int64_t);
void sr_emit_window(const at::Tensor&, const at::Tensor&,
                    const std::vector<at::Tensor>&, at::Tensor&, int64_t,
                    int64_t, int64_t, int64_t,
                    const std::vector<at::Tensor>&);
std::vector<at::Tensor> sr_emit_lanes_scratch(const at::Tensor&, int64_t,
                                              int64_t, int64_t);
void sr_emit_lanes(const at::Tensor&, const at::Tensor&,
                   const std::vector<at::Tensor>&, at::Tensor&,
                   const at::Tensor&, int64_t, int64_t, int64_t, int64_t,
                   const std::vector<at::Tensor>&);

// esim.hip
std::vector<at::Tensor> esim_scratch(const at::Tensor&, int64_t, int64_t);
void esim_count(const at::Tensor&, const at::Tensor&, const at::Tensor&,
                const at::Tensor&, int64_t, int64_t, double, double, double,
                const std::vector<at::Tensor>&, at::Tensor&);
void esim_scan(int64_t, const std::vector<at::Tensor>&, at::Tensor&);
std::vector<int64_t> esim_emit(const at::Tensor&, const at::Tensor&,
                               at::Tensor&, at::Tensor&, int64_t, int64_t,
                               double, double, double, int64_t,
                               const std::vector<at::Tensor>&);
void esim_sort(int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
               const std::vector<at::Tensor>&);
void esim_unpack(int64_t, const std::vector<at::Tensor>&,
                 const std::vector<at::Tensor>&);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("deform_conv2d_forward", &deform_conv2d_forward,
        "modulated deformable conv forward (gfx950)");
  m.def("deform_conv2d_backward", &deform_conv2d_backward,
        "modulated deformable conv backward (gfx950, batched)");
  m.def("deform_conv2d_forward_cols", &deform_conv2d_forward_cols,
        "im2col + GEMM forward; returns (out, cols) for the backward to reuse");
  m.def("deform_conv2d_backward_cols", &deform_conv2d_backward_cols,
        "backward with optional saved columns and a path selector "
        "(auto / fused / split)");
  m.def("deform_im2col", &deform_im2col_debug,
        "deformable im2col (test hook)");
  m.def("deform_conv2d_forward_fused", &deform_conv2d_forward_fused,
        "fused im2col+MFMA deformable conv forward (test hook)");
  m.def("gru_gates_ur_forward", &gru_gates_ur_forward);
  m.def("gru_gates_ur_backward", &gru_gates_ur_backward);
  m.def("gru_gates_out_forward", &gru_gates_out_forward);
  m.def("gru_gates_out_backward", &gru_gates_out_backward);
  m.def("splat_count", &splat_count);
  m.def("splat_stack", &splat_stack);
  m.def("grid_cap", &grid_cap,
        "work items one grid of a capped grid-stride kernel covers");
  m.def("conv2d_fwd_mfma", &conv2d_fwd_mfma,
        "bf16/fp16 NCHW conv fwd, MFMA implicit GEMM, fused bias+act (gfx950)");
  m.def("conv2d_fwd_valu", &conv2d_fwd_valu,
        "bf16/fp16 NCHW conv fwd, direct VALU, fused bias+act (gfx950)");
  m.def("conv2d_fwd_valu2", &conv2d_fwd_valu2,
        "bf16/fp16 NCHW conv fwd, register-strip VALU v2 for tiny channels");
  m.def("conv2d_dgrad_s2", &conv2d_dgrad_s2,
        "bf16 stride-2 conv input-grad (gfx950)");
  m.def("conv2d_wgrad_mfma", &conv2d_wgrad_mfma,
        "bf16 conv weight-grad, MFMA split-K + fp32 atomics (gfx950)");
  m.def("conv2d_s1", &conv2d_s1,
        "bf16/fp16 stride-1 3x3/1x1 conv, 8x32-tile MFMA core: forward with "
        "fused bias+act, or the input grad (dgrad=True) (gfx950)");
  m.def("conv2d_wgrad_s1", &conv2d_wgrad_s1,
        "bf16 stride-1 conv weight grad, deterministic two-stage reduction, "
        "dW [Cout,Cin,k,k] bf16 (gfx950)");
  m.def("act_grad", &act_grad, "fused activation backward (bf16/fp16)");
  m.def("act_grad_bias", &act_grad_bias,
        "activation backward + per-channel bias grad in one pass: "
        "{dpre, db}, with want_f32 also the fp32 sums; deterministic "
        "(bf16/fp16)",
        py::arg("dy"), py::arg("y"), py::arg("act"),
        py::arg("want_f32") = false);
  m.def("bias_grad", &bias_grad,
        "per-channel sum of an NCHW gradient: {db}, with want_f32 also the "
        "fp32 sums; deterministic (bf16/fp16)",
        py::arg("dy"), py::arg("want_f32") = false);
  m.def("bias_grad_chunk", &bias_grad_chunk,
        "elements of a channel one block of bias_grad sums");
  m.def("bias_grad_chain", &bias_grad_chain,
        "longest fp32 addition chain of bias_grad for (B, H, W)");
  m.def("gemm16_probe", &gemm16_probe, "16x16x32 bf16/fp16 MFMA fragment probe");
  m.def("redistribute_stack_hip", &redistribute_stack_hip,
        "count stack -> sorted event cloud, device-only "
        "(scan + scatter + segmented radix sort)");
  m.def("flat_grad_finite_check", &flat_grad_finite_check,
        "raise found_inf in the device state if the flat fp32 grad has "
        "inf/NaN");
  m.def("flat_adam_step", &flat_adam_step,
        "flat-buffer Adam/AdamW step with device-side un-scale and skip");
  m.def("flat_scale_update", &flat_scale_update,
        "GradScaler-style scale/step update of the device state");
  m.def("flat_grad_stats", &flat_grad_stats,
        "finite check plus deterministic fp64 sum of squares of the flat "
        "grad; writes grad norm, clip coefficient and clipped-step count");
  m.def("flat_adam_step_clipped", &flat_adam_step_clipped,
        "flat_adam_step with the gradient multiplied by the clip "
        "coefficient after un-scaling");
  m.def("stream_window_advance", &stream_window_advance,
        "per-stream sliding-window shift/reset of a [seqn,S,2,kH,kW] buffer, "
        "control read from a device tensor");
  m.def("stream_splat_ragged", &stream_splat_ragged,
        "splat concatenated per-stream LR event windows into the newest "
        "frame of a [seqn,S,2,kH,kW] buffer");
  m.def("evs_batch_splat", &evs_batch_splat,
        "splat a batch of packed event windows (jobs read from a device "
        "tensor) into [J,2,kH,kW] count planes, in place");
  m.def("evs_batch_splat_chunk", &evs_batch_splat_chunk,
        "events one block of evs_batch_splat covers");
  m.def("restoration_metrics", &restoration_metrics,
        "per-plane sum|p-t|, sum(p-t)^2, max t, min t and 7x7 SSIM sum of "
        "fp32 [P,H,W] maps, fp64 [P,5], deterministic");
  m.def("restoration_metrics_tile", &restoration_metrics_tile,
        "(TH, TW) pixel tile one block of restoration_metrics owns");
  m.def("sr_emit_scratch", &sr_emit_scratch,
        "scratch of sr_emit_window for (ncells, capacity), allocated once");
  m.def("sr_emit_counts", &sr_emit_counts,
        "the counts stage of sr_emit_window: NaN -> 0, else "
        "clamp(rint(v), 0, cell_cap), int32 (test hook)");
  m.def("sr_emit_window", &sr_emit_window,
        "append one predicted window [2,kH,kW] as sorted event rows to the "
        "typed chunk columns at a device cursor; int64 offsets, integer "
        "phases, float64 timestamps, overflow counted; capture-safe");
  m.def("sr_emit_lanes_scratch", &sr_emit_lanes_scratch,
        "scratch of sr_emit_lanes for (lanes, ncells, capacity_max), "
        "allocated once");
  m.def("sr_emit_lanes", &sr_emit_lanes,
        "sr_emit_window for S maps [S,2,kH,kW] at once: per-lane clocks, "
        "cursors, capacities and window indices, inactive lanes untouched; "
        "one scan and one sort for all lanes; capture-safe");
  m.def("esim_scratch", &esim_scratch,
        "scratch of the event simulator for (npix, capacity), allocated once");
  m.def("esim_count", &esim_count,
        "events per pixel over intervals k0+1..k0+nint of a float64 [S,H,W] "
        "slab of log frames, state untouched; stats = {total, largest "
        "crossing count, bad-input flag}");
  m.def("esim_scan", &esim_scan,
        "int64 exclusive sum of the simulator's counts and their total");
  m.def("esim_emit", &esim_emit,
        "the walk of esim_count, writing (tie-break key, t) per event and "
        "committing ref and t_last; returns {pix_bits, i_bits, key_bits}");
  m.def("esim_sort", &esim_sort,
        "0: sort by the tie-break key on the bits in use and make the "
        "pack_events words; 1: stable sort by the float64 timestamp");
  m.def("esim_unpack", &esim_unpack,
        "sorted (t, word) pairs -> uint16 x, uint16 y, float64 t, int8 p");
  m.attr("gfx_arch") = "gfx950";
}
