// C ABI over caffe::Net<float> (include/mscnn_net.h).  Every entry point catches caffe::FatalError (the
// CHECK-failure exception of this build) and returns it as an error string instead of aborting the host process.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/mscnn_hip.h"
#include "../../../include/mscnn_net.h"
#include "caffe/caffe.hpp"

using caffe::Blob;
using caffe::Caffe;
using caffe::Net;

struct mscnn_net {
  std::unique_ptr<Net<float> > net;
  int device;
  caffe::DeviceBuffer det_ws;
  caffe::DeviceBuffer img_in, img_ws;      // set_image: the uint8 frame and the resize scratch
  caffe::DeviceBuffer det_pack;            // detect: [count | dets | ids] in one allocation -> ONE D2H copy, one sync
  void* det_host = nullptr;                // host-coherent pinned memory: the blocking detect's pack (written by the kernels themselves)
  void* det_host_dev = nullptr;            // ... as the device addresses it
  size_t det_host_bytes = 0;
  std::vector<int> row_end;                // detect_image: end row of every image in the ROI blobs, of forward number rows_forward
  long rows_forward = -1;
  // detect_begin / detect_end: two pinned slots, each behind an event on the net's stream
  struct Slot { caffe::DeviceBuffer pack; void* host = nullptr; size_t bytes = 0; hipEvent_t done = nullptr; int cap = 0, handoff_errors = 0; } slot[2];
  int slot_head = 0, slot_tail = 0, slots_inflight = 0;
  // mscnn_net_set_nms: bbNms's knobs for every detect call from now on (pNms at the top of the reference scripts)
  mscnn_nms_params nms;
  bool nms_set = false;                    // false: the defaults -- the calls hand the ops NULL and run what they always ran
  // mscnn_net_set_box_voting: 0 = off (detect_merge_end enqueues what it always did), else the vote's overlap threshold in (0, 1)
  double vote_thr = 0.0;
  // mscnn_net_set_soft_nms: method 0 = off (detect_merge_end runs mscnn_detections_merge_fwd, as it always did), else the soft op's knobs
  mscnn_soft_nms_params soft = {0, 0.5, 0.001, 0};
  // mscnn_net_set_matrix_nms: method 0 = off, else detect_merge_end runs mscnn_detections_merge_matrix_fwd (never on together with soft)
  mscnn_matrix_nms_params matrix = {0, 0.5, 0.001, 0};
  // mscnn_net_set_wbf: thr 0 = off, else detect_merge_end runs mscnn_detections_merge_wbf_fwd (never on together with soft, matrix or
  // the vote); wbf_expected 0 = the views added to the frame's lists since _begin
  mscnn_wbf_params wbf = {0.0, 0.0, MSCNN_WBF_CONF_AVG, 0};
  int wbf_expected = 0;
  bool members_valid = false;              // the last detect_merge_end ran WBF and succeeded: wbf_members are its detections' counts
  std::vector<int> wbf_members, wbf_seg_dets;
  // mscnn_net_set_seq_nms: link_thr 0 = off, else detect_merge_end runs mscnn_detections_merge_seq_fwd over the lists as the frames of
  // one clip (never on together with soft, matrix or wbf; the vote runs behind it)
  mscnn_seq_nms_params seq = {0.0, 0.001, 300, MSCNN_SEQ_NMS_AVG, 0};
  bool sequences_valid = false;            // the last detect_merge_end ran Seq-NMS and succeeded: seq_ids are its detections' sequence ids
  std::vector<int> seq_ids, seq_seg_dets;
  // mscnn_net_set_tracker: off by default; while on, detect_multi / detect_cascade_multi / detect_merge_end enqueue
  // mscnn_tracks_update_fwd behind their pack.  Two state buffers: a call reads the committed one (track_cur) and writes the other, and
  // they are swapped only after the call has succeeded, so a call that is run twice (a hand-off recovery) or fails steps nothing.
  bool track_on = false;
  mscnn_track_params track = {0.5, 0.1, 0.5, 0.3, 0.5, 0.5, MSCNN_TRACK_MOTION_LINEAR, 30, 1};
  int track_max = 256;
  int track_K = 0;                         // slots per frame, fixed by the first call after a reset (0: not fixed, no state yet)
  int track_cur = 0;
  caffe::DeviceBuffer track_state[2];
  bool tracks_valid = false;               // the last tracked call succeeded: track_ids are its detections' track ids
  // mscnn_net_set_tracker_streams: the frames of a tracked call belong to track_streams streams (cameras), frame b to
  // track_stream_of[b] (mscnn_net_set_frame_streams, sticky); the table holds track_streams * track_K slots.  1: exactly as without.
  int track_streams = 1;
  std::vector<int> track_stream_of;
  std::vector<char> track_reset_pending;   // mscnn_net_tracker_reset_stream: streams to reset in front of the next tracked call's update
  std::vector<int> track_ids, track_seg_dets;
  // mscnn_net_set_tracker_kalman: a Kalman filter per track (the tracker on with motion none); the tracked calls run
  // mscnn_tracks_update_kalman_fwd, and a filter table stands beside each of the two track tables, swapped with them (track_cur).
  bool kalman_on = false;
  mscnn_track_kalman_params kalman = {1.0 / 20, 1.0 / 160, 1e-2, 1e-5, 1e-1, 1};
  // mscnn_net_set_tracker_assign: the matching of the two passes.  Optimal: the tracked calls run mscnn_tracks_update_assign_fwd on the
  // same tables (both forms read and write the same ones, so a switch touches nothing).
  int track_assign = MSCNN_TRACK_ASSIGN_GREEDY;
  caffe::DeviceBuffer track_filter[2];
  // mscnn_net_render: what the last detect_multi / detect_cascade_multi / detect_merge_end left in det_host -- the pack of `frames` x
  // `slots` segments with `cap` rows and, when that call ran the tracker, its ids at ids_at (bytes: both).  Any other user of det_host
  // ends it (ensure_det_host).  The stage's own device buffers: the pack's copy, the staged host frames, the frames to hand back.
  struct Render {
    bool valid = false, ids = false;
    int frames = 0, slots = 0, cap = 0;
    size_t bytes = 0, ids_at = 0;
    caffe::DeviceBuffer pack, in, out;
  } render;
  // mscnn_net_crops: the stage's own device buffers -- the staged host frames, the views op's workspace, the patches of a host `out`
  struct Crops { caffe::DeviceBuffer in, ws, out; } crops;
  // mscnn_net_detect_merge_*: the candidate lists of the forwards added since _begin (mscnn_hip.h: mscnn_detections_candidates_*)
  struct Merge {
    bool open = false;
    int images = 0, slots = 0, cand_cap = 0, passes = 0, handoff_errors = 0;      // slots: per image (classes, or outputs x classes)
    long rows = 0;                         // sum of R_all over the adds so far: the host-known bound on any list
    std::vector<double> overlap;           // per segment, from the first add that reached the segment's list
    std::vector<char> overlap_known;       // (the views adds may leave a list without an image for a while)
    std::vector<int> views;                // per frame: the views added to its lists since _begin (WBF's expected = 0)
    caffe::DeviceBuffer cand;
  } merge;
  ~mscnn_net() {
    if (det_host) (void)hipHostFree(det_host);
    for (Slot& sl : slot) {
      if (sl.done) { (void)hipEventSynchronize(sl.done); (void)hipEventDestroy(sl.done); }
      if (sl.host) (void)hipHostFree(sl.host);
    }
  }
};

namespace {
thread_local std::string g_err;

template <class F>
int guarded(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return 1;
  }
}

void fill_shape(const Blob<float>& b, int* dims8, int* ndim) {
  *ndim = b.num_axes();
  for (int i = 0; i < 8; ++i) dims8[i] = i < b.num_axes() ? b.shape(i) : 1;
}

int create(caffe::NetParameter param, int device, mscnn_net** out, unsigned flags = 0, bool use_default_fusion = true) {
  return guarded([&] {
    CHECK(out != nullptr);
    if (device >= 0) Caffe::SetDevice(device);   // device < 0: graph construction only (no HIP device touched)
    Caffe::set_mode(Caffe::GPU);
    std::unique_ptr<mscnn_net> h(new mscnn_net());
    h->device = device;
    if (use_default_fusion) h->net.reset(new Net<float>(param, caffe::TEST));
    else h->net.reset(new Net<float>(param, caffe::TEST, !(flags & MSCNN_NET_NO_FUSION)));
    *out = h.release();
  });
}
}  // namespace

extern "C" {

const char* mscnn_net_last_error(void) { return g_err.c_str(); }

int mscnn_net_create_from_file(const char* path, int device, mscnn_net** out) {
  caffe::NetParameter p;
  int rc = guarded([&] { caffe::ReadNetParamsFromTextFileOrDie(path, &p); });
  return rc ? rc : create(p, device, out);
}

int mscnn_net_create_from_string(const char* text, int device, mscnn_net** out) {
  caffe::NetParameter p;
  int rc = guarded([&] { p = caffe::NetParameterFromString(text); });
  return rc ? rc : create(p, device, out);
}

int mscnn_net_create_from_string_ex(const char* text, int device, unsigned flags, mscnn_net** out) {
  caffe::NetParameter p;
  int rc = guarded([&] { p = caffe::NetParameterFromString(text); });
  return rc ? rc : create(p, device, out, flags, false);
}

void mscnn_net_destroy(mscnn_net* net) { delete net; }

int mscnn_net_load_caffemodel(mscnn_net* net, const char* path) { return guarded([&] { net->net->CopyTrainedLayersFrom(path); }); }

int mscnn_net_set_stream(void* stream) { Caffe::set_stream(stream); return 0; }

int mscnn_net_num_layers(const mscnn_net* n) { return (int)n->net->layers().size(); }
const char* mscnn_net_layer_name(const mscnn_net* n, int i) { return n->net->layer_names()[i].c_str(); }
const char* mscnn_net_layer_type(const mscnn_net* n, int i) { return n->net->layers()[i]->type(); }
int mscnn_net_layer_index(const mscnn_net* n, const char* name) {
  const auto& v = n->net->layer_names();
  for (size_t i = 0; i < v.size(); ++i)
    if (v[i] == name) return (int)i;
  return -1;
}
int mscnn_net_layer_num_bottoms(const mscnn_net* n, int l) { return (int)n->net->bottom_vecs()[l].size(); }
int mscnn_net_layer_num_tops(const mscnn_net* n, int l) { return (int)n->net->top_vecs()[l].size(); }
static const char* blob_name_of(const mscnn_net* n, const Blob<float>* b) {
  const auto& blobs = n->net->blobs();
  for (size_t i = 0; i < blobs.size(); ++i)
    if (blobs[i].get() == b) return n->net->blob_names()[i].c_str();
  return "";
}
const char* mscnn_net_layer_bottom(const mscnn_net* n, int l, int i) { return blob_name_of(n, n->net->bottom_vecs()[l][i]); }
const char* mscnn_net_layer_top(const mscnn_net* n, int l, int i) { return blob_name_of(n, n->net->top_vecs()[l][i]); }
int mscnn_net_layer_num_params(const mscnn_net* n, int l) { return (int)n->net->layers()[l]->blobs().size(); }
int mscnn_net_layer_param_shape(const mscnn_net* n, int l, int p, int* dims8, int* ndim) {
  return guarded([&] {
    CHECK_LT(p, (int)n->net->layers()[l]->blobs().size());
    fill_shape(*n->net->layers()[l]->blobs()[p], dims8, ndim);
  });
}
const char* mscnn_net_layer_param_text(const mscnn_net* n, int l) {
  static thread_local std::string text;
  text = n->net->layers()[l]->layer_param().raw().DebugString();
  return text.c_str();
}
int mscnn_net_layer_fused_away(const mscnn_net* n, int l) { return n->net->layer_fused_away()[l] ? 1 : 0; }
const char* mscnn_net_layer_kernel(const mscnn_net* n, int l) {
  auto* c = dynamic_cast<caffe::ConvolutionLayer<float>*>(n->net->layers()[l].get());
  if (c) return c->kernel_name();
  auto* ip = dynamic_cast<caffe::InnerProductLayer<float>*>(n->net->layers()[l].get());
  if (ip) return ip->kernel_name();
  auto* ra = dynamic_cast<caffe::ROIAlignLayer<float>*>(n->net->layers()[l].get());
  return ra ? ra->kernel_name() : "";
}
int mscnn_net_set_inner_product_algo(mscnn_net* n, int layer, int algo) {
  return guarded([&] {
    CHECK_LT(layer, (int)n->net->layers().size());
    CHECK(algo == 0 || algo == 1) << "inner product algo: 0 auto, 1 gemm.hip's stream-K kernel";
    for (int l = (layer < 0 ? 0 : layer); l < (layer < 0 ? (int)n->net->layers().size() : layer + 1); ++l)
      if (auto* ip = dynamic_cast<caffe::InnerProductLayer<float>*>(n->net->layers()[l].get())) ip->set_algo(algo);
      else CHECK_LT(layer, 0) << "layer " << n->net->layer_names()[l] << " is not an InnerProduct";
  });
}
double mscnn_net_layer_flops(const mscnn_net* n, int l) { return n->net->layers()[l]->ForwardFlops(); }
static caffe::ConvolutionLayer<float>* conv_of(const mscnn_net* n, int l) {
  return dynamic_cast<caffe::ConvolutionLayer<float>*>(n->net->layers()[l].get());
}
double mscnn_net_layer_executed_flops(const mscnn_net* n, int l) {
  auto* c = conv_of(n, l);
  return c ? c->ExecutedFlops() : n->net->layers()[l]->ForwardFlops();
}
int mscnn_net_set_conv_profiling(mscnn_net* n, int on) {
  return guarded([&] {
    for (size_t l = 0; l < n->net->layers().size(); ++l)
      if (auto* c = conv_of(n, (int)l)) c->set_profiling(on != 0);
  });
}
int mscnn_net_layer_stage_ms(const mscnn_net* n, int l, float ms_out[3]) {
  ms_out[0] = ms_out[1] = ms_out[2] = 0.f;
  auto* c = conv_of(n, l);
  return (c && c->StageMs(ms_out)) ? 0 : 1;
}
int mscnn_net_set_conv_algo(mscnn_net* n, int layer, int algo) {
  return guarded([&] {
    CHECK_LT(layer, (int)n->net->layers().size());
    for (int l = (layer < 0 ? 0 : layer); l < (layer < 0 ? (int)n->net->layers().size() : layer + 1); ++l)
      if (auto* c = conv_of(n, l)) { c->set_algo(algo); c->set_calibrated_direct(false); }
      else CHECK_LT(layer, 0) << "layer " << n->net->layer_names()[l] << " is not a Convolution";
  });
}
int mscnn_net_set_conv_tuning(mscnn_net* n, int layer, int variant, int grid, int flags) {
  return guarded([&] {
    CHECK_LT(layer, (int)n->net->layers().size());
    for (int l = (layer < 0 ? 0 : layer); l < (layer < 0 ? (int)n->net->layers().size() : layer + 1); ++l)
      if (auto* c = conv_of(n, l)) c->set_tuning(variant, grid, flags);
  });
}
int mscnn_net_set_precision(mscnn_net* n, const char* dtype) {
  return guarded([&] {
    const std::string d = dtype ? dtype : "";
    CHECK(d == "f32" || d == "f16" || d == "f16x3") << "precision must be f32, f16 or f16x3, not '" << d << "'";
    for (size_t l = 0; l < n->net->layers().size(); ++l) {
      // (a layer the numerical calibration sent to the direct fp32 kernel stays there in the fp32-grade modes: the calibration is about
      // the data, not about the mode that happened to be active; the reduced-precision f16 mode has its own tolerance policy)
      if (auto* c = conv_of(n, (int)l)) c->set_algo(d == "f16" ? 4 : c->calibrated_direct() ? 1 : d == "f16x3" ? 5 : 0);
      if (auto* ip = dynamic_cast<caffe::InnerProductLayer<float>*>(n->net->layers()[l].get())) { ip->set_f16(d == "f16"); ip->set_x3(d == "f16x3"); }
    }
  });
}
const char* mscnn_net_layer_dtype(const mscnn_net* n, int l) {
  if (auto* c = conv_of(n, l)) return c->dtype();
  if (auto* ip = dynamic_cast<caffe::InnerProductLayer<float>*>(n->net->layers()[l].get())) return ip->dtype();
  return "f32";
}
int mscnn_net_calibrate_numerics(mscnn_net* n, double tol, int* num_switched) {
  return guarded([&] {
    const std::vector<int> sw = n->net->CalibrateNumerics(tol);
    if (num_switched) *num_switched = (int)sw.size();
  });
}
double mscnn_net_layer_calibration_err(const mscnn_net* n, int l) { return n->net->calibration_err()[l]; }
int mscnn_net_set_numerics_watch(mscnn_net* n, int period, double tol) {
  return guarded([&] {
    CHECK_GE(period, 0);
    n->net->SetNumericsWatch(period, tol);
  });
}
int mscnn_net_numerics_watch_state(const mscnn_net* n, int* checks, int* switched_layers, int cap) {
  const std::vector<int>& sw = n->net->numerics_watch_switched();
  if (checks) *checks = n->net->numerics_watch_checks();
  for (int i = 0; switched_layers && i < cap && i < (int)sw.size(); ++i) switched_layers[i] = sw[i];
  return (int)sw.size();
}
int mscnn_net_set_auto_calibrate(mscnn_net* n, double tol) {
  return guarded([&] { n->net->SetAutoCalibrate(tol); });
}
int mscnn_net_set_chain_fusion(mscnn_net* n, int on) {
  return guarded([&] { n->net->SetChainFusion(on != 0); });
}
int mscnn_net_set_boxoutput_one_pass(mscnn_net* n, int on) {
  return guarded([&] {
    for (const auto& layer : n->net->layers())
      if (auto* bo = dynamic_cast<caffe::BoxOutputLayer<float>*>(layer.get())) bo->set_one_pass(on != 0);
  });
}
int mscnn_net_set_roialign_one_pass(mscnn_net* n, int on) {
  return guarded([&] { n->net->SetRoiAlignOnePass(on != 0); });
}
int mscnn_net_roialign_pairs(const mscnn_net* n, int* first_layers, int cap) {
  const std::vector<int> heads = n->net->roialign_pairs();
  for (int i = 0; first_layers && i < cap && i < (int)heads.size(); ++i) first_layers[i] = heads[i];
  return (int)heads.size();
}
int mscnn_net_chain_pairs(const mscnn_net* n, int* producers, int* consumers, int cap) {
  const auto pairs = n->net->chain_pairs();
  for (int i = 0; i < cap && i < (int)pairs.size(); ++i) {
    if (producers) producers[i] = pairs[i].first;
    if (consumers) consumers[i] = pairs[i].second;
  }
  return (int)pairs.size();
}
int mscnn_net_auto_calibrate_state(const mscnn_net* n, int* checks, int* switched_layers, int cap) {
  const std::vector<int>& sw = n->net->auto_calibrate_switched();
  if (checks) *checks = n->net->auto_calibrate_checks();
  for (int i = 0; switched_layers && i < cap && i < (int)sw.size(); ++i) switched_layers[i] = sw[i];
  return (int)sw.size();
}
int mscnn_net_num_blobs(const mscnn_net* n) { return (int)n->net->blobs().size(); }
const char* mscnn_net_blob_name(const mscnn_net* n, int b) { return n->net->blob_names()[b].c_str(); }
int mscnn_net_blob_shape(const mscnn_net* n, const char* name, int* dims8, int* ndim) {
  return guarded([&] {
    CHECK(n->net->has_blob(name)) << "Unknown blob name " << name;
    fill_shape(*n->net->blob_by_name(name), dims8, ndim);
  });
}
int mscnn_net_num_inputs(const mscnn_net* n) { return n->net->num_inputs(); }
int mscnn_net_num_outputs(const mscnn_net* n) { return n->net->num_outputs(); }
const char* mscnn_net_output_name(const mscnn_net* n, int i) { return n->net->blob_names()[n->net->output_blob_indices()[i]].c_str(); }

int mscnn_net_set_param(mscnn_net* n, int l, int p, const float* host, size_t count) {
  return guarded([&] {
    auto& blobs = n->net->layers()[l]->blobs();
    CHECK_LT(p, (int)blobs.size());
    CHECK_EQ((size_t)blobs[p]->count(), count) << "param size mismatch for layer " << n->net->layer_names()[l];
    n->net->MaterializeStale();      // (intermediate blobs a chained forward left unwritten: the old weights' outputs, written before they change)
    std::memcpy(blobs[p]->mutable_cpu_data(), host, sizeof(float) * count);
    n->net->layers()[l]->OnWeightsChanged();
  });
}
int mscnn_net_get_param(mscnn_net* n, int l, int p, float* host, size_t count) {
  return guarded([&] {
    auto& blobs = n->net->layers()[l]->blobs();
    CHECK_LT(p, (int)blobs.size());
    CHECK_EQ((size_t)blobs[p]->count(), count);
    std::memcpy(host, blobs[p]->cpu_data(), sizeof(float) * count);
  });
}

int mscnn_net_set_blob(mscnn_net* n, const char* name, const float* host, size_t count) {
  return guarded([&] {
    CHECK(n->net->has_blob(name)) << "Unknown blob name " << name;
    n->net->MaterializePendingReadersOf(name);      // (a deferred ROI pooling that reads this blob writes its own blob first)
    auto b = n->net->blob_by_name(name);
    CHECK_EQ((size_t)b->count(), count) << "blob " << name << " has shape " << b->shape_string();
    std::memcpy(b->mutable_cpu_data(), host, sizeof(float) * count);
  });
}
int mscnn_net_set_blob_device(mscnn_net* n, const char* name, const float* dev, size_t count) {
  return guarded([&] {
    CHECK(n->net->has_blob(name)) << "Unknown blob name " << name;
    n->net->MaterializePendingReadersOf(name);      // (a deferred ROI pooling that reads this blob writes its own blob first)
    auto b = n->net->blob_by_name(name);
    CHECK_EQ((size_t)b->count(), count) << "blob " << name << " has shape " << b->shape_string();
    HIP_CHECK(hipMemcpyAsync(b->mutable_gpu_data(), dev, sizeof(float) * count, hipMemcpyDeviceToDevice, (hipStream_t)Caffe::stream()));
  });
}
int mscnn_net_set_image(mscnn_net* n, const char* name, const unsigned char* img_rgb, int on_device, int org_h, int org_w,
                        const float* mean_bgr) {
  return guarded([&] {
    CHECK(n->net->has_blob(name)) << "Unknown blob name " << name;
    n->net->MaterializePendingReadersOf(name);      // (blobs the last forward left unwritten that hang on this blob are written first, as in the other setters)
    auto b = n->net->blob_by_name(name);
    CHECK(b->num() == 1 && b->channels() == 3) << "set_image: blob " << name << " has shape " << b->shape_string();
    hipStream_t st = (hipStream_t)Caffe::stream();
    const unsigned char* dev_img = img_rgb;
    if (!on_device) {
      const size_t bytes = (size_t)org_h * org_w * 3;
      void* d = n->img_in.Reserve(bytes);
      HIP_CHECK(hipMemcpyAsync(d, img_rgb, bytes, hipMemcpyHostToDevice, st));
      dev_img = static_cast<const unsigned char*>(d);
    }
    const size_t wb = mscnn_preprocess_workspace_bytes(org_h, org_w, b->height(), b->width());
    void* ws = n->img_ws.Reserve(wb);
    static const float kMean[3] = {104.f, 117.f, 123.f};      // run_mscnn_detection.m:38
    const int rc = mscnn_preprocess_u8_f32(dev_img, org_h, org_w, b->mutable_gpu_data(), b->height(), b->width(),
                                           mean_bgr ? mean_bgr : kMean, ws, wb, st);
    CHECK_EQ(rc, 0) << mscnn_last_error();
  });
}
int mscnn_net_set_images(mscnn_net* n, const char* name, const unsigned char* const* imgs_rgb, int on_device, const int* org_h,
                         const int* org_w, int count, const float* mean_bgr) {
  return guarded([&] {
    CHECK(n->net->has_blob(name)) << "Unknown blob name " << name;
    auto b = n->net->blob_by_name(name);
    CHECK(b->num_axes() == 4 && b->channels() == 3) << "set_images: blob " << name << " has shape " << b->shape_string();
    CHECK(count == b->num()) << "set_images: " << count << " images for blob " << name << " of shape " << b->shape_string();
    CHECK(imgs_rgb && org_h && org_w) << "set_images: null pointer";
    const int H = b->height(), W = b->width();
    for (int i = 0; i < count; ++i)
      CHECK(imgs_rgb[i] && org_h[i] > 0 && org_w[i] > 0) << "set_images: image " << i << " is " << org_h[i] << " x " << org_w[i]
                                                          << (imgs_rgb[i] ? "" : " at a null pointer");
    n->net->MaterializePendingReadersOf(name);      // (as set_image)
    hipStream_t st = (hipStream_t)Caffe::stream();
    std::vector<const unsigned char*> dev(imgs_rgb, imgs_rgb + count);
    if (!on_device) {                               // staged back to back into img_in (256-byte aligned offsets)
      std::vector<size_t> off(count + 1, 0);
      for (int i = 0; i < count; ++i) off[i + 1] = off[i] + (((size_t)org_h[i] * org_w[i] * 3 + 255) & ~(size_t)255);
      unsigned char* d = static_cast<unsigned char*>(n->img_in.Reserve(off[count]));
      for (int i = 0; i < count; ++i) {
        HIP_CHECK(hipMemcpyAsync(d + off[i], imgs_rgb[i], (size_t)org_h[i] * org_w[i] * 3, hipMemcpyHostToDevice, st));
        dev[i] = d + off[i];
      }
    }
    const size_t wb = mscnn_preprocess_batch_workspace_bytes(count, org_h, org_w, H, W);
    void* ws = n->img_ws.Reserve(wb);
    static const float kMean[3] = {104.f, 117.f, 123.f};      // run_mscnn_detection.m:38
    const int rc = mscnn_preprocess_batch_u8_f32(dev.data(), org_h, org_w, count, b->mutable_gpu_data(), H, W,
                                                 mean_bgr ? mean_bgr : kMean, ws, wb, st);
    CHECK_EQ(rc, 0) << mscnn_last_error();
  });
}
int mscnn_net_set_image_views(mscnn_net* n, const char* name, const unsigned char* const* frames_rgb, int on_device, const int* org_h,
                              const int* org_w, int num_frames, const mscnn_preprocess_view* views, int count, const float* mean_bgr) {
  return guarded([&] {
    CHECK(n->net->has_blob(name)) << "Unknown blob name " << name;
    auto b = n->net->blob_by_name(name);
    CHECK(b->num_axes() == 4 && b->channels() == 3) << "set_image_views: blob " << name << " has shape " << b->shape_string();
    CHECK(count == b->num()) << "set_image_views: " << count << " views for blob " << name << " of shape " << b->shape_string();
    CHECK(frames_rgb && org_h && org_w && views) << "set_image_views: null pointer";
    CHECK_GE(num_frames, 1) << "set_image_views: num_frames " << num_frames;
    const int H = b->height(), W = b->width();
    for (int f = 0; f < num_frames; ++f)
      CHECK(frames_rgb[f] && org_h[f] > 0 && org_w[f] > 0) << "set_image_views: frame " << f << " is " << org_h[f] << " x " << org_w[f]
                                                          << (frames_rgb[f] ? "" : " at a null pointer");
    for (int v = 0; v < count; ++v) {      // (the op refuses the same: here nothing has been uploaded yet)
      const mscnn_preprocess_view& q = views[v];
      CHECK(q.frame >= 0 && q.frame < num_frames) << "set_image_views: view " << v << ": frame " << q.frame << " outside [0, " << num_frames << ")";
      CHECK(q.w >= 1 && q.h >= 1 && q.x0 >= 0 && q.y0 >= 0 && (long)q.x0 + q.w <= (long)org_w[q.frame] && (long)q.y0 + q.h <= (long)org_h[q.frame])
          << "set_image_views: view " << v << ": window " << q.h << " x " << q.w << " (h x w) at (x0 " << q.x0 << ", y0 " << q.y0
          << ") is empty or not inside frame " << q.frame << " of " << org_h[q.frame] << " x " << org_w[q.frame];
      CHECK(q.flip_x == 0 || q.flip_x == 1) << "set_image_views: view " << v << ": flip_x " << q.flip_x << " (0 or 1)";
    }
    CHECK_GE(n->device, 0) << "set_image_views: the net was built with device " << n->device << " (graph only)";
    n->net->MaterializePendingReadersOf(name);      // (as set_image)
    hipStream_t st = (hipStream_t)Caffe::stream();
    std::vector<const unsigned char*> dev(frames_rgb, frames_rgb + num_frames);
    if (!on_device) {                               // every frame once, whatever the number of its views (256-byte aligned offsets)
      std::vector<size_t> off(num_frames + 1, 0);
      for (int f = 0; f < num_frames; ++f) off[f + 1] = off[f] + (((size_t)org_h[f] * org_w[f] * 3 + 255) & ~(size_t)255);
      unsigned char* d = static_cast<unsigned char*>(n->img_in.Reserve(off[num_frames]));
      for (int f = 0; f < num_frames; ++f) {
        HIP_CHECK(hipMemcpyAsync(d + off[f], frames_rgb[f], (size_t)org_h[f] * org_w[f] * 3, hipMemcpyHostToDevice, st));
        dev[f] = d + off[f];
      }
    }
    const size_t wb = mscnn_preprocess_views_workspace_bytes(views, count, H, W);
    void* ws = n->img_ws.Reserve(wb);
    static const float kMean[3] = {104.f, 117.f, 123.f};      // run_mscnn_detection.m:38
    const int rc = mscnn_preprocess_views_u8_f32(dev.data(), org_h, org_w, num_frames, views, count, b->mutable_gpu_data(), H, W,
                                                 mean_bgr ? mean_bgr : kMean, ws, wb, st);
    CHECK_EQ(rc, 0) << mscnn_last_error();
  });
}
int mscnn_net_get_blob(mscnn_net* n, const char* name, float* host, size_t capacity, size_t* count) {
  return guarded([&] {
    CHECK(n->net->has_blob(name)) << "Unknown blob name " << name;
    auto b = n->net->blob_by_name(name);
    const float* src = b->cpu_data();      // (synchronises the stream)
    if (n->net->HandoffRecover()) {        // a hand-off timed out in the forward this blob comes from: the Net has run it again
      b = n->net->blob_by_name(name);
      src = b->cpu_data();
    }
    if (count) *count = (size_t)b->count();
    CHECK_LE((size_t)b->count(), capacity) << "buffer too small for blob " << name;
    std::memcpy(host, src, sizeof(float) * b->count());
  });
}
const float* mscnn_net_blob_device_ptr(mscnn_net* n, const char* name) {
  const float* p = nullptr;
  guarded([&] {
    CHECK(n->net->has_blob(name)) << "Unknown blob name " << name;
    p = n->net->blob_by_name(name)->gpu_data();
  });
  return p;
}

int mscnn_net_forward(mscnn_net* n) { return guarded([&] { n->net->Forward(); }); }
int mscnn_net_forward_from_to(mscnn_net* n, int from, int to) {
  return guarded([&] { n->net->ForwardFromTo(from, to < 0 ? (int)n->net->layers().size() - 1 : to); });
}
int mscnn_net_reshape(mscnn_net* n) { return guarded([&] { n->net->Reshape(); }); }
int mscnn_net_handoff_state(const mscnn_net* n, int* whole_tiles_forced) {
  if (whole_tiles_forced) *whole_tiles_forced = mscnn_wgemm_whole_tiles_forced();
  return n->net->handoff_errors();
}
int mscnn_net_set_layer_timing(mscnn_net* n, int on) { n->net->set_layer_timing(on != 0); return 0; }
float mscnn_net_layer_ms(const mscnn_net* n, int l) { return n->net->layer_ms()[l]; }

// What the detect calls hand to the ops: NULL for the defaults.  The cascade calls carry their own det_thr argument; a setting
// whose det_thr (the plain stage's, mscnn_net.h) is set is refused there by name, as the ops refuse it -- never ignored.
static const mscnn_nms_params* nms_arg(const mscnn_net* n, bool cascade) {
  if (!n->nms_set) return nullptr;
  CHECK(!cascade || n->nms.det_thr == 0.f) << "the net's nms setting has det_thr " << n->nms.det_thr << ", which is the plain stage's: the "
                                              "cascade calls take det_thr as an argument (mscnn_net_set_nms with det_thr = 0)";
  return &n->nms;
}

int mscnn_net_set_nms(mscnn_net* n, const mscnn_nms_params* nms) {
  return guarded([&] {
    CHECK(n != nullptr);
    mscnn_nms_params r, dflt;
    MSCNN_CHECK(mscnn_nms_params_resolve(nms, &r));      // (refuses 'ms' / 'cover' / 'none' and out-of-range fields, naming the value)
    MSCNN_CHECK(mscnn_nms_params_resolve(nullptr, &dflt));
    n->nms = r;
    n->nms_set = std::memcmp(&r, &dflt, sizeof(r)) != 0;
  });
}

int mscnn_net_get_nms(const mscnn_net* n, mscnn_nms_params* out) {
  return guarded([&] {
    CHECK(n && out);
    if (n->nms_set) *out = n->nms;
    else MSCNN_CHECK(mscnn_nms_params_resolve(nullptr, out));
  });
}

int mscnn_net_set_box_voting(mscnn_net* n, double thr) {
  return guarded([&] {
    CHECK(n != nullptr);
    CHECK(thr == 0.0 || (thr > 0.0 && thr < 1.0)) << "set_box_voting: thr " << thr << " is neither 0 (off) nor inside (0, 1)";
    CHECK(thr == 0.0 || n->wbf.thr == 0.0) << "set_box_voting: thr " << thr << " while weighted boxes fusion is on (set_wbf thr " << n->wbf.thr
                                           << "): the two exclude each other, turn that one off first";
    n->vote_thr = thr == 0.0 ? 0.0 : thr;      // (-0.0 is off too)
  });
}

int mscnn_net_get_box_voting(const mscnn_net* n, double* thr) {
  return guarded([&] {
    CHECK(n && thr);
    *thr = n->vote_thr;
  });
}

int mscnn_net_set_soft_nms(mscnn_net* n, int method, double sigma, double score_thr, int max_out) {
  return guarded([&] {
    CHECK(n != nullptr);
    // (the op's own refusals, made here so that a refused value changes nothing and is named at the call that brought it)
    CHECK(method == 0 || method == MSCNN_SOFT_NMS_LINEAR || method == MSCNN_SOFT_NMS_GAUSSIAN)
        << "set_soft_nms: method " << method << " is neither 0 (off), " << MSCNN_SOFT_NMS_LINEAR << " (linear) nor " << MSCNN_SOFT_NMS_GAUSSIAN
        << " (gaussian)";
    CHECK(method != MSCNN_SOFT_NMS_GAUSSIAN || (sigma > 0 && sigma < HUGE_VAL)) << "set_soft_nms: sigma " << sigma << " is not a finite value > 0";
    CHECK(score_thr >= 0 && score_thr < HUGE_VAL) << "set_soft_nms: score_thr " << score_thr << " is not a finite value >= 0";
    CHECK_GE(max_out, 0) << "set_soft_nms: max_out " << max_out;
    CHECK(method == 0 || n->matrix.method == 0) << "set_soft_nms: method " << method << " while Matrix NMS is on (set_matrix_nms method "
                                                << n->matrix.method << "): the two exclude each other, turn that one off first";
    CHECK(method == 0 || n->wbf.thr == 0.0) << "set_soft_nms: method " << method << " while weighted boxes fusion is on (set_wbf thr "
                                            << n->wbf.thr << "): the two exclude each other, turn that one off first";
    CHECK(method == 0 || n->seq.link_thr == 0.0) << "set_soft_nms: method " << method << " while Seq-NMS is on (set_seq_nms link_thr "
                                                 << n->seq.link_thr << "): the two exclude each other, turn that one off first";
    n->soft = mscnn_soft_nms_params{method, sigma, score_thr, max_out};
  });
}

int mscnn_net_get_soft_nms(const mscnn_net* n, int* method, double* sigma, double* score_thr, int* max_out) {
  return guarded([&] {
    CHECK(n && method && sigma && score_thr && max_out);
    *method = n->soft.method; *sigma = n->soft.sigma; *score_thr = n->soft.score_thr; *max_out = n->soft.max_out;
  });
}

int mscnn_net_set_matrix_nms(mscnn_net* n, int method, double sigma, double score_thr, int max_out) {
  return guarded([&] {
    CHECK(n != nullptr);
    // (the op's own refusals, made here so that a refused value changes nothing and is named at the call that brought it)
    CHECK(method == 0 || method == MSCNN_MATRIX_NMS_LINEAR || method == MSCNN_MATRIX_NMS_GAUSSIAN)
        << "set_matrix_nms: method " << method << " is neither 0 (off), " << MSCNN_MATRIX_NMS_LINEAR << " (linear) nor "
        << MSCNN_MATRIX_NMS_GAUSSIAN << " (gaussian)";
    CHECK(method != MSCNN_MATRIX_NMS_GAUSSIAN || (sigma > 0 && sigma < HUGE_VAL)) << "set_matrix_nms: sigma " << sigma << " is not a finite value > 0";
    CHECK(score_thr >= 0 && score_thr < HUGE_VAL) << "set_matrix_nms: score_thr " << score_thr << " is not a finite value >= 0";
    CHECK_GE(max_out, 0) << "set_matrix_nms: max_out " << max_out;
    CHECK(method == 0 || n->soft.method == 0) << "set_matrix_nms: method " << method << " while Soft-NMS is on (set_soft_nms method "
                                              << n->soft.method << "): the two exclude each other, turn that one off first";
    CHECK(method == 0 || n->wbf.thr == 0.0) << "set_matrix_nms: method " << method << " while weighted boxes fusion is on (set_wbf thr "
                                            << n->wbf.thr << "): the two exclude each other, turn that one off first";
    CHECK(method == 0 || n->seq.link_thr == 0.0) << "set_matrix_nms: method " << method << " while Seq-NMS is on (set_seq_nms link_thr "
                                                 << n->seq.link_thr << "): the two exclude each other, turn that one off first";
    n->matrix = mscnn_matrix_nms_params{method, sigma, score_thr, max_out};
  });
}

int mscnn_net_get_matrix_nms(const mscnn_net* n, int* method, double* sigma, double* score_thr, int* max_out) {
  return guarded([&] {
    CHECK(n && method && sigma && score_thr && max_out);
    *method = n->matrix.method; *sigma = n->matrix.sigma; *score_thr = n->matrix.score_thr; *max_out = n->matrix.max_out;
  });
}

int mscnn_net_set_wbf(mscnn_net* n, double thr, double skip_thr, int conf_type, int expected, int max_out) {
  return guarded([&] {
    CHECK(n != nullptr);
    // (the op's own refusals, made here so that a refused value changes nothing and is named at the call that brought it)
    CHECK(thr == 0.0 || (thr > 0.0 && thr < 1.0)) << "set_wbf: thr " << thr << " is neither 0 (off) nor inside (0, 1)";
    CHECK(skip_thr >= 0 && skip_thr < HUGE_VAL) << "set_wbf: skip_thr " << skip_thr << " is not a finite value >= 0";
    CHECK(conf_type == MSCNN_WBF_CONF_AVG || conf_type == MSCNN_WBF_CONF_MAX)
        << "set_wbf: conf_type " << conf_type << " is neither " << MSCNN_WBF_CONF_AVG << " (avg) nor " << MSCNN_WBF_CONF_MAX << " (max)";
    CHECK_GE(expected, 0) << "set_wbf: expected " << expected << " is neither 0 (the views added) nor >= 1";
    CHECK_GE(max_out, 0) << "set_wbf: max_out " << max_out;
    const bool on = thr != 0.0;
    CHECK(!on || n->soft.method == 0) << "set_wbf: thr " << thr << " while Soft-NMS is on (set_soft_nms method " << n->soft.method
                                      << "): the two exclude each other, turn that one off first";
    CHECK(!on || n->matrix.method == 0) << "set_wbf: thr " << thr << " while Matrix NMS is on (set_matrix_nms method " << n->matrix.method
                                        << "): the two exclude each other, turn that one off first";
    CHECK(!on || n->vote_thr == 0.0) << "set_wbf: thr " << thr << " while box voting is on (set_box_voting thr " << n->vote_thr
                                     << "): the two exclude each other, turn that one off first";
    CHECK(!on || n->seq.link_thr == 0.0) << "set_wbf: thr " << thr << " while Seq-NMS is on (set_seq_nms link_thr " << n->seq.link_thr
                                         << "): the two exclude each other, turn that one off first";
    CHECK(!on || !n->track_on) << "set_wbf: thr " << thr << " while the tracker is on (set_tracker high_thr " << n->track.high_thr
                               << "): the two exclude each other (the track ids go where WBF's member counts go), turn that one off first";
    n->wbf = mscnn_wbf_params{on ? thr : 0.0, skip_thr, conf_type, max_out};      // (-0.0 is off too)
    n->wbf_expected = expected;
  });
}

int mscnn_net_get_wbf(const mscnn_net* n, double* thr, double* skip_thr, int* conf_type, int* expected, int* max_out) {
  return guarded([&] {
    CHECK(n && thr && skip_thr && conf_type && expected && max_out);
    *thr = n->wbf.thr; *skip_thr = n->wbf.skip_thr; *conf_type = n->wbf.conf_type; *expected = n->wbf_expected; *max_out = n->wbf.max_out;
  });
}

int mscnn_net_set_seq_nms(mscnn_net* n, double link_thr, double score_thr, int top_k, int rescore, int max_out) {
  return guarded([&] {
    CHECK(n != nullptr);
    // (the op's own refusals, made here so that a refused value changes nothing and is named at the call that brought it)
    CHECK(link_thr == 0.0 || (link_thr > 0.0 && link_thr < 1.0)) << "set_seq_nms: link_thr " << link_thr << " is neither 0 (off) nor inside (0, 1)";
    CHECK(score_thr >= 0 && score_thr < HUGE_VAL) << "set_seq_nms: score_thr " << score_thr << " is not a finite value >= 0";
    CHECK(top_k >= 1 && top_k <= 1024) << "set_seq_nms: top_k " << top_k << " is outside [1, 1024]";
    CHECK(rescore == MSCNN_SEQ_NMS_AVG || rescore == MSCNN_SEQ_NMS_MAX)
        << "set_seq_nms: rescore " << rescore << " is neither " << MSCNN_SEQ_NMS_AVG << " (avg) nor " << MSCNN_SEQ_NMS_MAX << " (max)";
    CHECK_GE(max_out, 0) << "set_seq_nms: max_out " << max_out;
    const bool on = link_thr != 0.0;
    CHECK(!on || n->soft.method == 0) << "set_seq_nms: link_thr " << link_thr << " while Soft-NMS is on (set_soft_nms method " << n->soft.method
                                      << "): the two exclude each other, turn that one off first";
    CHECK(!on || n->matrix.method == 0) << "set_seq_nms: link_thr " << link_thr << " while Matrix NMS is on (set_matrix_nms method "
                                        << n->matrix.method << "): the two exclude each other, turn that one off first";
    CHECK(!on || n->wbf.thr == 0.0) << "set_seq_nms: link_thr " << link_thr << " while weighted boxes fusion is on (set_wbf thr " << n->wbf.thr
                                    << "): the two exclude each other, turn that one off first";
    CHECK(!on || !n->track_on || n->track_streams == 1)
        << "set_seq_nms: link_thr " << link_thr << " while the tracker has " << n->track_streams
        << " streams (set_tracker_streams): a clip links list t to list t - 1, so it is one stream; set that one to 1 first";
    n->seq = mscnn_seq_nms_params{on ? link_thr : 0.0, score_thr, top_k, rescore, max_out};      // (-0.0 is off too)
  });
}

int mscnn_net_get_seq_nms(const mscnn_net* n, double* link_thr, double* score_thr, int* top_k, int* rescore, int* max_out) {
  return guarded([&] {
    CHECK(n && link_thr && score_thr && top_k && rescore && max_out);
    *link_thr = n->seq.link_thr; *score_thr = n->seq.score_thr; *top_k = n->seq.top_k; *rescore = n->seq.rescore; *max_out = n->seq.max_out;
  });
}

int mscnn_net_set_tracker(mscnn_net* n, const mscnn_track_params* p, int max_tracks) {
  return guarded([&] {
    CHECK(n != nullptr);
    if (p == nullptr) {      // off: the state is dropped with the setting
      n->track_on = false; n->track_K = 0; n->tracks_valid = false; n->kalman_on = false; n->track_assign = MSCNN_TRACK_ASSIGN_GREEDY;
      n->track_streams = 1; n->track_stream_of.clear(); n->track_reset_pending.clear();
      return;
    }
    // (the op's own refusals, made here so that a refused value changes nothing and is named at the call that brought it)
    CHECK(max_tracks >= 1 && max_tracks <= 1024) << "set_tracker: max_tracks " << max_tracks << " is outside [1, 1024]";
    CHECK(!(p->high_thr != p->high_thr) && !(p->low_thr != p->low_thr) && !(p->new_thr != p->new_thr))
        << "set_tracker: a NaN threshold (high_thr " << p->high_thr << ", low_thr " << p->low_thr << ", new_thr " << p->new_thr << ")";
    CHECK(p->match_thr >= 0 && p->match_thr < 1) << "set_tracker: match_thr " << p->match_thr << " is not inside [0, 1)";
    CHECK(p->match_thr_low >= 0 && p->match_thr_low < 1) << "set_tracker: match_thr_low " << p->match_thr_low << " is not inside [0, 1)";
    CHECK(p->low_thr <= p->high_thr) << "set_tracker: low_thr " << p->low_thr << " is above high_thr " << p->high_thr;
    CHECK(p->new_thr >= p->high_thr) << "set_tracker: new_thr " << p->new_thr << " is below high_thr " << p->high_thr;
    CHECK(p->vel_gain > 0 && p->vel_gain <= 1) << "set_tracker: vel_gain " << p->vel_gain << " is not inside (0, 1]";
    CHECK(p->motion == MSCNN_TRACK_MOTION_NONE || p->motion == MSCNN_TRACK_MOTION_LINEAR)
        << "set_tracker: motion " << p->motion << " is neither " << MSCNN_TRACK_MOTION_NONE << " (none) nor " << MSCNN_TRACK_MOTION_LINEAR << " (linear)";
    CHECK_GE(p->max_age, 0) << "set_tracker: max_age " << p->max_age;
    CHECK_GE(p->min_hits, 1) << "set_tracker: min_hits " << p->min_hits;
    CHECK(n->wbf.thr == 0.0) << "set_tracker: high_thr " << p->high_thr << " while weighted boxes fusion is on (set_wbf thr " << n->wbf.thr
                             << "): the two exclude each other (the track ids go where WBF's member counts go), turn that one off first";
    n->track = *p; n->track_max = max_tracks; n->track_on = true;
    n->track_K = 0; n->tracks_valid = false;      // a new setting is a new stream: the next call starts at id 1
    n->track_streams = 1; n->track_stream_of.clear(); n->track_reset_pending.clear();      // (and ONE stream: mscnn_net_set_tracker_streams)
    n->kalman_on = false;      // (and no filter: mscnn_net_set_tracker_kalman)
    n->track_assign = MSCNN_TRACK_ASSIGN_GREEDY;      // (and the greedy walk: mscnn_net_set_tracker_assign)
  });
}

int mscnn_net_set_tracker_assign(mscnn_net* n, int method) {
  return guarded([&] {
    CHECK(n != nullptr);
    CHECK(n->track_on) << "set_tracker_assign: the tracker is off (mscnn_net_set_tracker)";
    CHECK(method == MSCNN_TRACK_ASSIGN_GREEDY || method == MSCNN_TRACK_ASSIGN_OPTIMAL)
        << "set_tracker_assign: assign " << method << " is neither " << MSCNN_TRACK_ASSIGN_GREEDY << " (greedy) nor " << MSCNN_TRACK_ASSIGN_OPTIMAL
        << " (optimal)";
    n->track_assign = method;      // (the tables, the streams, the mapping and the filter stay: the next call goes on from them)
  });
}

int mscnn_net_get_tracker_assign(const mscnn_net* n, int* method) {
  return guarded([&] {
    CHECK(n && method);
    *method = n->track_on ? n->track_assign : 0;
  });
}

int mscnn_net_set_tracker_streams(mscnn_net* n, int num_streams) {
  return guarded([&] {
    CHECK(n != nullptr);
    CHECK(n->track_on) << "set_tracker_streams: the tracker is off (mscnn_net_set_tracker)";
    CHECK(num_streams >= 1 && num_streams <= 256) << "set_tracker_streams: num_streams " << num_streams << " is outside [1, 256]";
    CHECK(num_streams == 1 || n->seq.link_thr == 0.0)
        << "set_tracker_streams: num_streams " << num_streams << " while Seq-NMS is on (set_seq_nms link_thr " << n->seq.link_thr
        << "): a clip links list t to list t - 1, so it is one stream; turn that one off first";
    n->track_streams = num_streams;
    n->track_stream_of.clear(); n->track_reset_pending.clear();
    n->track_K = 0; n->tracks_valid = false;      // a fresh table, K unfixed (as mscnn_net_tracker_reset)
  });
}

int mscnn_net_set_tracker_kalman(mscnn_net* n, const mscnn_track_kalman_params* p) {
  return guarded([&] {
    CHECK(n != nullptr);
    if (p != nullptr) {
      CHECK(n->track_on) << "set_tracker_kalman: the tracker is off (mscnn_net_set_tracker)";
      CHECK(n->track.motion == MSCNN_TRACK_MOTION_NONE)
          << "set_tracker_kalman: the tracker's motion " << n->track.motion << " is not " << MSCNN_TRACK_MOTION_NONE
          << " (none): the filter is the motion, set the tracker with motion none first";
      const double stds[5] = {p->std_position, p->std_velocity, p->std_aspect, p->std_aspect_velocity, p->std_aspect_measure};
      const char* const names[5] = {"std_position", "std_velocity", "std_aspect", "std_aspect_velocity", "std_aspect_measure"};
      for (int i = 0; i < 5; ++i)      // (NaN included)
        CHECK(stds[i] > 0 && stds[i] <= 1.7976931348623157e308) << "set_tracker_kalman: " << names[i] << " " << stds[i] << " is not a finite number above 0";
      n->kalman = *p;
    }
    if (p == nullptr && !n->kalman_on) return;      // (off while it is off: nothing changes, the tracks live on)
    n->kalman_on = p != nullptr;
    n->track_reset_pending.clear();
    n->track_K = 0; n->tracks_valid = false;      // a fresh table, K unfixed (as mscnn_net_set_tracker_streams); streams and mapping stay
  });
}

int mscnn_net_get_tracker_kalman(const mscnn_net* n, int* on, mscnn_track_kalman_params* p) {
  return guarded([&] {
    CHECK(n && on && p);
    *on = n->kalman_on ? 1 : 0; *p = n->kalman;
  });
}

int mscnn_net_tracker_kalman_state(mscnn_net* n, void* filter_host, size_t bytes) {
  return guarded([&] {
    CHECK(n != nullptr);
    CHECK(n->track_on && n->kalman_on) << "tracker_kalman_state: the filter is off (mscnn_net_set_tracker_kalman)";
    CHECK(n->track_K >= 1) << "tracker_kalman_state: no tracked call has succeeded since the tracker was set or reset: the number of slots is not fixed yet";
    const size_t need = mscnn_tracks_kalman_state_bytes(n->track_streams * n->track_K, n->track_max);
    CHECK(filter_host != nullptr && bytes >= need) << "tracker_kalman_state: a buffer of " << bytes << " bytes, " << n->track_streams * n->track_K
                                                    << " slots x " << n->track_max << " tracks need " << need;
    hipStream_t st = (hipStream_t)Caffe::stream();
    HIP_CHECK(hipMemcpyAsync(filter_host, n->track_filter[n->track_cur].get(), need, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

int mscnn_net_set_frame_streams(mscnn_net* n, const int* stream_of, int count) {
  return guarded([&] {
    CHECK(n != nullptr);
    if (stream_of == nullptr || count == 0) { n->track_stream_of.clear(); return; }
    CHECK(n->track_on) << "set_frame_streams: the tracker is off (mscnn_net_set_tracker)";
    CHECK(count >= 1 && count <= 256) << "set_frame_streams: count " << count << " is outside [0, 256]";
    for (int b = 0; b < count; ++b)
      CHECK(stream_of[b] >= 0 && stream_of[b] < n->track_streams)
          << "set_frame_streams: stream_of[" << b << "] = " << stream_of[b] << " is outside [0, " << n->track_streams
          << ") (mscnn_net_set_tracker_streams)";
    n->track_stream_of.assign(stream_of, stream_of + count);
  });
}

int mscnn_net_get_tracker_streams(const mscnn_net* n, int* num_streams, int* stream_of, int cap, int* count) {
  return guarded([&] {
    CHECK(n && num_streams && count);
    const int c = (int)n->track_stream_of.size();
    CHECK(c == 0 || (stream_of != nullptr && cap >= c)) << "get_tracker_streams: the buffer holds " << cap << " entries, the mapping has " << c;
    *num_streams = n->track_streams; *count = c;
    for (int b = 0; b < c; ++b) stream_of[b] = n->track_stream_of[b];
  });
}

int mscnn_net_tracker_reset_stream(mscnn_net* n, int s) {
  return guarded([&] {
    CHECK(n != nullptr);
    CHECK(n->track_on) << "tracker_reset_stream: the tracker is off (mscnn_net_set_tracker)";
    CHECK(s >= 0 && s < n->track_streams) << "tracker_reset_stream: stream " << s << " is outside [0, " << n->track_streams << ")";
    if (n->track_K == 0) return;      // (no table yet: the first tracked call makes a fresh one)
    // the reset itself runs on the net's stream in front of the next tracked call's update, on the committed table: resetting a
    // table twice is resetting it once, so a body that runs twice resets and steps what one run does; cleared by the commit
    n->track_reset_pending.resize(n->track_streams, 0);
    n->track_reset_pending[s] = 1;
  });
}

int mscnn_net_get_tracker(const mscnn_net* n, int* on, mscnn_track_params* p, int* max_tracks, int* num_slots) {
  return guarded([&] {
    CHECK(n && on && p && max_tracks && num_slots);
    *on = n->track_on ? 1 : 0; *p = n->track; *max_tracks = n->track_max; *num_slots = n->track_K;
  });
}

int mscnn_net_tracker_reset(mscnn_net* n) {
  return guarded([&] {
    CHECK(n != nullptr);
    CHECK(n->track_on) << "tracker_reset: the tracker is off (mscnn_net_set_tracker)";
    n->track_K = 0; n->tracks_valid = false;      // (the next tracked call resets the table on its stream, in front of its update)
    n->track_reset_pending.clear();
  });
}

int mscnn_net_tracker_state(mscnn_net* n, void* state_host, size_t bytes) {
  return guarded([&] {
    CHECK(n != nullptr);
    CHECK(n->track_on) << "tracker_state: the tracker is off (mscnn_net_set_tracker)";
    CHECK(n->track_K >= 1) << "tracker_state: no tracked call has succeeded since the tracker was set or reset: the number of slots is not fixed yet";
    const size_t need = mscnn_tracks_state_layout_of(n->track_streams * n->track_K, n->track_max).total;
    CHECK(state_host != nullptr && bytes >= need) << "tracker_state: a buffer of " << bytes << " bytes, " << n->track_streams * n->track_K
                                                   << " slots x " << n->track_max << " tracks need " << need;
    hipStream_t st = (hipStream_t)Caffe::stream();
    HIP_CHECK(hipMemcpyAsync(state_host, n->track_state[n->track_cur].get(), need, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

int mscnn_net_detect_tracks(mscnn_net* n, int* ids_host, int cap, const int* seg_dets) {
  return guarded([&] {
    CHECK(n != nullptr);
    CHECK(n->tracks_valid) << "detect_tracks: the last detect call did not run the tracker (mscnn_net_set_tracker was off, the call failed, "
                              "or there was none)";
    CHECK(seg_dets != nullptr) << "detect_tracks: null seg_dets";
    const size_t S = n->track_seg_dets.size();
    for (size_t s = 0; s < S; ++s)
      CHECK_EQ(seg_dets[s], n->track_seg_dets[s]) << "detect_tracks: segment " << s << ": seg_dets " << seg_dets[s] << ", that call returned "
                                                  << n->track_seg_dets[s];
    const size_t D = n->track_ids.size();
    CHECK_LE(D, (size_t)(cap < 0 ? 0 : cap)) << "detect_tracks: the buffer holds " << cap << " ids, that call returned " << D << " detections";
    CHECK(D == 0 || ids_host) << "detect_tracks: null id buffer";
    if (D) std::memcpy(ids_host, n->track_ids.data(), D * sizeof(int));
  });
}

// The single-segment and the asynchronous forms leave no place for a frame's track ids: refused while the tracker is on, so that no
// frame of the stream goes by untracked without a word.
static void track_refuses(const mscnn_net* n, const char* name) {
  CHECK(!n->track_on) << name << ": refused while the tracker is on (set_tracker high_thr " << n->track.high_thr
                      << "): only detect_multi, detect_cascade_multi and detect_merge_end step the tracks; turn the tracker off first";
}
// K of a tracked call against the K the first call after a reset fixed, and with several streams its T frames against the mapping;
// before anything is enqueued
static void track_slots_checked(const mscnn_net* n, const char* name, int T, int K) {
  CHECK(!n->track_on || n->track_K == 0 || n->track_K == K)
      << name << ": " << K << " slots per frame, the tracker's table was made for " << n->track_K
      << " by the first call after its reset (mscnn_net_tracker_reset starts a new stream)";
  CHECK(!n->track_on || n->track_streams == 1 || (int)n->track_stream_of.size() == T)
      << name << ": " << T << " frames, the mapping of frames to the tracker's " << n->track_streams << " streams names "
      << n->track_stream_of.size() << " (mscnn_net_set_frame_streams)";
}
// mscnn_tracks_update_fwd behind the pack of T frames x K slots with pack_rows rows at `pack` (device-addressable), ids to ids_dev:
// reads the committed table, writes the other one.  The first call after a reset makes and resets the tables, on the same stream.
static void track_enqueue(mscnn_net* n, const char* name, int T, int K, const void* pack, int pack_rows, int* ids_dev) {
  track_slots_checked(n, name, T, K);
  hipStream_t st = (hipStream_t)Caffe::stream();
  const int N = n->track_streams;
  CHECK_LE((long)N * (long)K, 0x7fffffffL) << name << ": " << N << " streams x " << K << " slots";
  const size_t bytes = mscnn_tracks_state_bytes(N * K, n->track_max);
  CHECK_GT(bytes, 0u) << name << ": the tracker's table for " << N * K << " slots x " << n->track_max << " tracks";
  if (n->track_K == 0) {
    for (caffe::DeviceBuffer& b : n->track_state) b.Reserve(bytes);
    if (n->kalman_on)      // (no reset: a filter record is made at its track's birth)
      for (caffe::DeviceBuffer& b : n->track_filter) b.Reserve(mscnn_tracks_kalman_state_bytes(N * K, n->track_max));
    MSCNN_CHECK(mscnn_tracks_state_reset(n->track_state[n->track_cur].get(), N * K, n->track_max, st));
  } else {
    for (size_t s = 0; s < n->track_reset_pending.size(); ++s)      // mscnn_net_tracker_reset_stream, on the committed table
      if (n->track_reset_pending[s])
        MSCNN_CHECK(mscnn_tracks_state_reset_slots(n->track_state[n->track_cur].get(), N * K, n->track_max, (int)s * K, K, st));
  }
  if (n->track_assign == MSCNN_TRACK_ASSIGN_OPTIMAL) {
    mscnn_tracks_assign_call c = {};
    c.size = sizeof(c); c.track = &n->track; c.filter = n->kalman_on ? &n->kalman : nullptr; c.assign = n->track_assign;
    c.num_frames = T; c.num_slots = K; c.num_streams = N; c.stream_of = N > 1 ? n->track_stream_of.data() : nullptr;
    c.pack_dev = pack; c.cap = pack_rows;
    c.state_in = n->track_state[n->track_cur].get(); c.state_out = n->track_state[n->track_cur ^ 1].get();
    if (n->kalman_on) { c.filter_in = n->track_filter[n->track_cur].get(); c.filter_out = n->track_filter[n->track_cur ^ 1].get(); }
    c.max_tracks = n->track_max; c.track_ids_dev = ids_dev; c.stream = st;
    MSCNN_CHECK(mscnn_tracks_update_assign_fwd(&c));
  } else if (n->kalman_on) {
    mscnn_tracks_kalman_call c = {};
    c.size = sizeof(c); c.track = &n->track; c.filter = &n->kalman;
    c.num_frames = T; c.num_slots = K; c.num_streams = N; c.stream_of = N > 1 ? n->track_stream_of.data() : nullptr;
    c.pack_dev = pack; c.cap = pack_rows;
    c.state_in = n->track_state[n->track_cur].get(); c.state_out = n->track_state[n->track_cur ^ 1].get();
    c.filter_in = n->track_filter[n->track_cur].get(); c.filter_out = n->track_filter[n->track_cur ^ 1].get();
    c.max_tracks = n->track_max; c.track_ids_dev = ids_dev; c.stream = st;
    MSCNN_CHECK(mscnn_tracks_update_kalman_fwd(&c));
  } else if (N == 1)
    MSCNN_CHECK(mscnn_tracks_update_fwd(&n->track, T, K, pack, pack_rows, n->track_state[n->track_cur].get(),
                                        n->track_state[n->track_cur ^ 1].get(), n->track_max, ids_dev, st));
  else
    MSCNN_CHECK(mscnn_tracks_update_streams_fwd(&n->track, T, K, N, n->track_stream_of.data(), pack, pack_rows,
                                                n->track_state[n->track_cur].get(), n->track_state[n->track_cur ^ 1].get(), n->track_max,
                                                ids_dev, st));
}
// the call has succeeded: the table it wrote is the committed one
static void track_commit(mscnn_net* n, int K) { n->track_cur ^= 1; n->track_K = K; n->track_reset_pending.clear(); }

size_t mscnn_net_detect_pack_bytes(int cap) {
  const size_t rows = (size_t)(cap > 0 ? cap : 1);
  return (16 + rows * (5 * sizeof(double) + sizeof(int)) + 15) / 16 * 16;
}

// Final stage into the fixed-capacity device pack [count, R, cap, 0 | cap x 5 doubles | cap ints]; no host transfer.
// [row0, row0 + rows) of the ROI blobs (rows < 0: all of them -- the batch-1 form)
// the net's host-side landing place for packs: host-coherent pinned memory, also addressable by the device (det_host_dev)
static void ensure_det_host(mscnn_net* n, size_t total) {
  n->render.valid = false;      // (the block is about to be written again: mscnn_net_render has nothing to read until a call says so)
  if (n->det_host_bytes >= total) return;
  if (n->det_host) HIP_CHECK(hipHostFree(n->det_host));
  n->det_host = nullptr; n->det_host_bytes = 0; n->det_host_dev = nullptr;
  HIP_CHECK(hipHostMalloc(&n->det_host, total, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent));
  HIP_CHECK(hipHostGetDevicePointer(&n->det_host_dev, n->det_host, 0));
  n->det_host_bytes = total;
}

// pack_at: a device-visible address to write the pack to instead of a device buffer (host-coherent pinned memory: the kernels only ever
// WRITE the pack, so the blocking mscnn_net_detect lets them write straight into the host's copy)
static void detect_into_pack(mscnn_net* n, const mscnn_detect_params* p, int cap, int* R_out, bool with_header, int row0 = 0, int nrows = -1,
                             caffe::DeviceBuffer* pack_buf = nullptr, char* pack_at = nullptr) {
  caffe::DeviceBuffer& det_pack = pack_buf ? *pack_buf : n->det_pack;
  CHECK(p != nullptr);
  CHECK(n->net->has_blob("bbox_pred") && n->net->has_blob("cls_pred") && n->net->has_blob("proposals_score"))
      << "net has no bbox_pred / cls_pred / proposals_score outputs";
  auto bbox = n->net->blob_by_name("bbox_pred");
  auto cls = n->net->blob_by_name("cls_pred");
  auto props = n->net->blob_by_name("proposals_score");
  const int R_all = props->num();
  CHECK_EQ(bbox->num(), R_all);
  CHECK_EQ(cls->num(), R_all);
  if (nrows < 0) {
    // the MATLAB stage is written for one image (run_mscnn_detection.m:75-120 runs on the outputs of a batch-1 forward): the NMS
    // must never mix boxes of different images
    if (n->net->num_inputs() > 0 && n->net->input_blobs()[0]->num_axes() == 4)
      CHECK_EQ(n->net->input_blobs()[0]->num(), 1) << "the net's input holds " << n->net->input_blobs()[0]->num()
                                                   << " images: use mscnn_net_detect_image (one final stage per image)";
    row0 = 0; nrows = R_all;
  }
  CHECK(row0 >= 0 && nrows >= 0 && row0 + nrows <= R_all);
  const int R = nrows;
  const int per_row_cls = R_all > 0 ? cls->count() / R_all : 1, per_row_box = R_all > 0 ? bbox->count() / R_all : 4;
  if (with_header && R > cap) {
    // Multi-GPU pack: a rank that fails here alone would leave the others blocked in the all_gather.  Mark the overflow in the header
    // {-1, R, cap, 0} and take part in the exchange: mscnn_net_unpack_detections then fails on EVERY rank, naming the numbers.
    char* pk = static_cast<char*>(det_pack.Reserve(mscnn_net_detect_pack_bytes(cap)));
    hipStream_t s0 = (hipStream_t)Caffe::stream();
    int* h = reinterpret_cast<int*>(pk);
    const int words[4] = {-1, R, cap, 0};
    MSCNN_CHECK(mscnn_store_words_i32(h, words, 4, s0));
    if (R_out) *R_out = R;
    return;
  }
  CHECK_LE(R, cap) << "detection pack capacity " << cap << " < " << R << " ROIs (size it by BoxOutput's max_nms_num)";
  mscnn_detections_desc d;
  d.ncls = per_row_cls;
  if (R_all > 0) CHECK_EQ(per_row_box, 4 * d.ncls);
  d.cls_id = p->cls_id;
  for (int k = 0; k < 4; ++k) { d.bbox_mean[k] = p->bbox_mean[k]; d.bbox_std[k] = p->bbox_std[k]; }
  d.proposal_thr = p->proposal_thr;
  d.ratio_h = p->ratio_h; d.ratio_w = p->ratio_w; d.org_h = p->org_h; d.org_w = p->org_w; d.nms_overlap = p->nms_overlap;
  const size_t wb = mscnn_detections_workspace_bytes(R);
  void* ws = n->det_ws.Reserve(wb);
  const size_t rows = (size_t)(cap > 0 ? cap : 1), total = mscnn_net_detect_pack_bytes(cap);
  char* pack = pack_at ? pack_at : static_cast<char*>(det_pack.Reserve(total));
  int* hdr = reinterpret_cast<int*>(pack);
  double* dets = reinterpret_cast<double*>(pack + 16);
  int* ids = reinterpret_cast<int*>(pack + 16 + sizeof(double) * 5 * rows);
  hipStream_t st = (hipStream_t)Caffe::stream();
  // header {count (written by the kernels), R, cap, 0}: only the multi-GPU pack needs R / cap on the device -- two 4-byte fills
  if (with_header) {
    const int words[3] = {R, cap, 0};
    MSCNN_CHECK(mscnn_store_words_i32(hdr + 1, words, 3, st));      // (one launch; three 4-byte memsets were three)
  }
  MSCNN_CHECK(mscnn_detections_nms_fwd(&d, nms_arg(n, false), bbox->gpu_data() + (size_t)row0 * per_row_box,
                                       cls->gpu_data() + (size_t)row0 * per_row_cls, props->gpu_data() + (size_t)row0 * 6, R, dets, ids,
                                       hdr, ws, wb, st));
  if (R_out) *R_out = R;
}

// End row of every image in ROI rows grouped by image: BoxOutput emits image after image (box_output_layer.cpp:107), column 0 of every
// row is its image (:156; DecodeBBox copies it).  Image i owns rows [end[i - 1], end[i]).
static std::vector<int> image_ranges(const float* host_props, int R, int stride, int num_images, const std::string& what) {
  std::vector<int> end(num_images, 0);
  int prev = 0;
  for (int r = 0; r < R; ++r) {
    const int img = (int)host_props[(size_t)r * stride];
    CHECK(img >= prev && img < num_images) << what << " are not grouped by image";
    // (the dummy row [0 0 0 0 0 0] the layer emits when nothing survives in the whole batch carries score 0 and image 0)
    prev = img;
    end[img] = r + 1;
  }
  for (int i = 1; i < num_images; ++i) if (end[i] < end[i - 1]) end[i] = end[i - 1];
  return end;
}

// Row range of image `image` in the ROI blobs.  One small D2H read of the proposals blob per forward (cached until the next forward).
static void image_rows(mscnn_net* n, int image, int* row0, int* rows) {
  CHECK(n->net->has_blob("proposals_score")) << "net has no proposals_score output";
  auto props = n->net->blob_by_name("proposals_score");
  const int num = n->net->num_inputs() > 0 ? n->net->input_blobs()[0]->num() : 1;
  CHECK(image >= 0 && image < num) << "image " << image << " of a batch of " << num;
  if (n->rows_forward != n->net->forward_count() || (int)n->row_end.size() != num) {
    n->row_end = image_ranges(props->cpu_data(), props->num(), 6, num, "proposals");      // (cpu_data synchronises the stream)
    n->rows_forward = n->net->forward_count();
  }
  *row0 = image > 0 ? n->row_end[image - 1] : 0;
  *rows = n->row_end[image] - *row0;
}

int mscnn_net_detect_device(mscnn_net* n, const mscnn_detect_params* p, int cap, const void** pack_dev) {
  return guarded([&] {
    CHECK(pack_dev != nullptr);
    track_refuses(n, "detect_device");
    detect_into_pack(n, p, cap, nullptr, true);
    *pack_dev = n->det_pack.get();
  });
}

// ---- the final stage of a STREAM of frames: frame i's detections travel to the host under frame i + 1's trunk ----------------------
int mscnn_net_detect_begin(mscnn_net* n, const mscnn_detect_params* p, int cap) {
  return guarded([&] {
    track_refuses(n, "detect_begin");
    CHECK(n->slots_inflight < 2) << "detect_begin: two frames already in flight (call mscnn_net_detect_end)";
    mscnn_net::Slot& sl = n->slot[n->slot_head];
    detect_into_pack(n, p, cap, nullptr, true, 0, -1, &sl.pack);      // (a device pack per slot: its copy may still run when the next frame's stage starts)
    const size_t total = mscnn_net_detect_pack_bytes(cap);
    if (sl.bytes < total) {
      if (sl.host) HIP_CHECK(hipHostFree(sl.host));
      sl.host = nullptr; sl.bytes = 0;
      HIP_CHECK(hipHostMalloc(&sl.host, total, hipHostMallocDefault));
      sl.bytes = total;
    }
    if (!sl.done) HIP_CHECK(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    hipStream_t st = (hipStream_t)Caffe::stream();
    // (the copy stays in the compute stream: on a stream of its own, beside the next frame's first kernels, it measured the same --
    // 224.85 against 224.83 images/s over 300 frames, tools/sessions/r06_s8.sh -- and needed a device pack per slot to be safe)
    HIP_CHECK(hipMemcpyAsync(sl.host, sl.pack.get(), total, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipEventRecord(sl.done, st));
    sl.cap = cap;
    sl.handoff_errors = n->net->handoff_errors();      // (an event of THIS frame's trunk was answered inside its forward, before this point)
    n->slot_head ^= 1;
    ++n->slots_inflight;
  });
}

int mscnn_net_detect_end(mscnn_net* n, double* dets_host, int* ids_host, int cap, int* num_dets, int* num_rois) {
  return guarded([&] {
    CHECK(n->slots_inflight > 0) << "detect_end: nothing in flight";
    mscnn_net::Slot& sl = n->slot[n->slot_tail];
    CHECK_EQ(sl.cap, cap) << "detect_end: the oldest frame in flight was begun with another capacity";
    HIP_CHECK(hipEventSynchronize(sl.done));
    n->slot_tail ^= 1;
    --n->slots_inflight;
    // A stream-K hand-off that timed out since the last look may have poisoned a tile of THIS frame or of the one enqueued behind it,
    // and neither can be run again from here (the input blob already holds a later frame): whole-tile scheduling is forced for the
    // process as everywhere else, and the caller is told to submit its last two frames again.
    // (the event may also have been noticed already -- and counted -- by the NEXT frame's forward, behind its BoxOutput read: that forward
    // restarted itself, but this frame's pack had left the device by then)
    const bool seen_now = n->net->HandoffEventSeen();
    CHECK(!seen_now && n->net->handoff_errors() == sl.handoff_errors) << "a stream-K hand-off timed out while frames were in flight (mscnn_net_handoff_state): whole-tile "
                                          "scheduling from now on; the frames begun since the last mscnn_net_detect_end must be submitted again";
    const int rc = mscnn_net_unpack_detections(sl.host, cap, dets_host, ids_host, num_dets, num_rois);
    CHECK_EQ(rc, 0) << g_err;
  });
}

int mscnn_net_unpack_detections(const void* pack_host, int cap, double* dets_host, int* ids_host, int* num_dets, int* num_rois) {
  return guarded([&] {
    CHECK(pack_host && num_dets);
    const char* hp = static_cast<const char*>(pack_host);
    const int* hdr = reinterpret_cast<const int*>(hp);
    const int D = hdr[0], R = hdr[1];
    CHECK_EQ(hdr[2], cap) << "detection pack was written for another capacity";
    CHECK(D != -1) << "detection pack capacity " << cap << " < " << R << " ROIs on the rank that wrote this pack (size it by BoxOutput's max_nms_num)";
    CHECK(D >= 0 && D <= R && R <= cap) << "corrupt detection pack: " << D << " detections, " << R << " ROIs, capacity " << cap;
    const size_t rows = (size_t)(cap > 0 ? cap : 1);
    if (D > 0 && dets_host) std::memcpy(dets_host, hp + 16, sizeof(double) * 5 * D);
    if (D > 0 && ids_host) std::memcpy(ids_host, hp + 16 + sizeof(double) * 5 * rows, sizeof(int) * D);
    *num_dets = D;
    if (num_rois) *num_rois = R;
  });
}

int mscnn_net_detect(mscnn_net* n, const mscnn_detect_params* p, double* dets_host, int* ids_host, int cap, int* num_dets,
                     int* num_rois) {
  return guarded([&] {
    CHECK(p && dets_host && num_dets);
    track_refuses(n, "detect");
    // single-GPU form: the pack is sized by this image's ROI count (16 + 44 R bytes) and -- round 6 -- lives in host-coherent pinned
    // memory that the final stage's kernels write directly (they only ever store into the pack): no D2H copy behind them, the host
    // waits for the stream and reads.  (An in-stream copy cost ~11 us of copy-engine start-up + its own time per frame:
    // profiles/r06_kernel_gaps.txt.)  Above 4032 ROIs -- the tiled path, whose kernels are not audited for that -- the pack stays on
    // the device and is copied as before.
    int R = 0, rows = 0;
    hipStream_t st = (hipStream_t)Caffe::stream();
    auto run = [&]() {
      rows = n->net->has_blob("proposals_score") ? n->net->blob_by_name("proposals_score")->num() : 0;
      const size_t total = mscnn_net_detect_pack_bytes(rows);
      ensure_det_host(n, total);
      if (rows >= 1 && rows <= 4032) {
        *static_cast<volatile int*>(n->det_host) = -1;
        detect_into_pack(n, p, rows, &R, false, 0, -1, nullptr, static_cast<char*>(n->det_host_dev));
      } else {
        detect_into_pack(n, p, rows, &R, false);
        HIP_CHECK(hipMemcpyAsync(n->det_host, n->det_pack.get(), total, hipMemcpyDeviceToHost, st));
      }
      HIP_CHECK(hipStreamSynchronize(st));
    };
    run();
    // a stream-K hand-off of roi_c1 / fc6 timed out in the forward these detections come from (mscnn_net_handoff_state): the Net has
    // run the frame again on whole tiles -- redo this stage on the new outputs
    if (n->net->HandoffRecover()) run();
    const char* hp = static_cast<const char*>(n->det_host);
    const int Dd = *reinterpret_cast<const int*>(hp);
    CHECK_LE(Dd, cap) << "detections buffer too small";
    CHECK_LE(Dd, rows);
    const size_t prow = (size_t)(rows > 0 ? rows : 1);
    if (Dd > 0) {
      std::memcpy(dets_host, hp + 16, sizeof(double) * 5 * Dd);
      if (ids_host) std::memcpy(ids_host, hp + 16 + sizeof(double) * 5 * prow, sizeof(int) * Dd);
    }
    *num_dets = Dd;
    if (num_rois) *num_rois = R;
  });
}

int mscnn_net_detect_image(mscnn_net* n, const mscnn_detect_params* p, int image, double* dets_host, int* ids_host, int cap,
                           int* num_dets, int* num_rois) {
  return guarded([&] {
    CHECK(p && dets_host && num_dets);
    track_refuses(n, "detect_image");
    int row0 = 0, rows = 0, R = 0;
    image_rows(n, image, &row0, &rows);
    if (n->net->HandoffRecover()) image_rows(n, image, &row0, &rows);      // (image_rows synchronised the stream: see mscnn_net_handoff_state)
    hipStream_t st = (hipStream_t)Caffe::stream();
    size_t total = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
      detect_into_pack(n, p, rows, &R, false, row0, rows);
      total = mscnn_net_detect_pack_bytes(rows);
      ensure_det_host(n, total);
      HIP_CHECK(hipMemcpyAsync(n->det_host, n->det_pack.get(), total, hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
      if (attempt == 1 || !n->net->HandoffRecover()) break;
      image_rows(n, image, &row0, &rows);      // the frame has been run again on whole tiles: once more on the new outputs
    }
    const char* hp = static_cast<const char*>(n->det_host);
    const int Dd = *reinterpret_cast<const int*>(hp);
    CHECK_LE(Dd, cap) << "detections buffer too small";
    CHECK_LE(Dd, rows);
    const size_t prow = (size_t)(rows > 0 ? rows : 1);
    if (Dd > 0) {
      std::memcpy(dets_host, hp + 16, sizeof(double) * 5 * Dd);
      if (ids_host) {
        std::memcpy(ids_host, hp + 16 + sizeof(double) * 5 * prow, sizeof(int) * Dd);
        for (int i = 0; i < Dd; ++i) ids_host[i] += row0;      // rows of the net's ROI blobs, not of the image's range
      }
    }
    *num_dets = Dd;
    if (num_rois) *num_rois = R;
  });
}

// ---- every (image, class) segment of the last forward in one pass ------------------------------------------------------------------
// Bound on any image's ROI rows, known on the host: the row bound of the BoxOutput layer that wrote proposals_score (its max_nms_num /
// max_post_nms_num, or its anchor count), per image.  Without such a layer: all rows.
static int per_image_row_bound(mscnn_net* n, int num_images, int R_all) {
  const auto& layers = n->net->layers();
  const Blob<float>* props = n->net->blob_by_name("proposals_score").get();
  for (size_t l = 0; l < layers.size(); ++l) {
    auto* bo = dynamic_cast<caffe::BoxOutputLayer<float>*>(layers[l].get());
    const auto& tops = n->net->top_vecs()[l];
    if (bo && tops.size() == 2 && tops[1] == props && bo->max_rows() > 0) {
      // (rows handed in through mscnn_net_forward_rois need not respect the layer's own per-image bound: their largest image counts)
      if (bo->max_image_rows() > 0) return std::min(R_all, bo->max_image_rows());
      return std::min(R_all, std::max(1, bo->max_rows() / num_images));
    }
  }
  return R_all;
}

// One source of segments: the plain stage's bbox_pred / cls_pred / proposals_score, or one cascade output's blob triple.
struct SegSource { const Blob<float>* boxes; const Blob<float>* cls; const Blob<float>* props; int ncls; bool cascade; };

// The multi pack of the last forward (mscnn_hip.h: mscnn_detections_multi_fwd) with cap rows for desc[num_images x sources x C], at
// pack_at (device-addressable) or in the net's device pack.  Returns false when it went to the device pack instead: a per-image bound
// over 4032 rows (max_nms_num 0) runs the per-call op -- the tiled kernels of nms_large.h -- segment after segment on row ranges read
// on the host (proposals_score's through image_rows' cache, one read per cascade output), into the same layout.
static bool segments_into_pack(mscnn_net* n, const std::vector<SegSource>& src, const std::vector<mscnn_detections_desc>& desc,
                               int num_images, int C, float det_thr, int cap, char* pack_at, char** pack_out) {
  const int O = (int)src.size(), K = O * C, S = num_images * K, R_all = src[0].props->num();
  hipStream_t st = (hipStream_t)Caffe::stream();
  const mscnn_multi_pack_layout L = mscnn_multi_pack_layout_of(S, cap);
  const int bound = n->net->has_blob("proposals_score") ? per_image_row_bound(n, num_images, R_all) : R_all;
  const mscnn_nms_params* nms = nms_arg(n, src[0].cascade);
  if (bound <= 4032) {
    const size_t wb = mscnn_detections_multi_workspace_bytes(S, bound);
    void* ws = n->det_ws.Reserve(wb);
    char* pack = pack_at ? pack_at : static_cast<char*>(n->det_pack.Reserve(L.total));
    if (src[0].cascade) {
      std::vector<mscnn_cascade_output> outs(O);
      for (int o = 0; o < O; ++o)
        outs[o] = mscnn_cascade_output{src[o].boxes->gpu_data(), src[o].cls->gpu_data(), src[o].props->gpu_data(), src[o].ncls};
      MSCNN_CHECK(mscnn_detections_cascade_multi_nms_fwd(desc.data(), det_thr, nms, num_images, O, C, outs.data(), R_all, bound, pack, cap, ws,
                                                         wb, st));
    } else {
      MSCNN_CHECK(mscnn_detections_multi_nms_fwd(desc.data(), nms, num_images, C, src[0].boxes->gpu_data(), src[0].cls->gpu_data(),
                                                 src[0].props->gpu_data(), R_all, bound, pack, cap, ws, wb, st));
    }
    *pack_out = pack;
    return pack == pack_at;
  }
  // (the per-segment path: lists over 4032 rows run the tiled kernels, which refuse a non-default nms setting, naming the limit)
  std::vector<std::vector<int> > end(O);
  int max_rows = 0;
  for (int o = 0; o < O; ++o) {
    if (src[o].cascade) {
      end[o] = image_ranges(src[o].props->cpu_data(), R_all, 5, num_images, "the proposals of cascade output " + std::to_string(o));
    } else {
      int r0 = 0, nr = 0;
      image_rows(n, 0, &r0, &nr);
      end[o] = n->row_end;
    }
    for (int i = 0; i < num_images; ++i) max_rows = std::max(max_rows, end[o][i] - (i > 0 ? end[o][i - 1] : 0));
  }
  char* pack = static_cast<char*>(n->det_pack.Reserve(L.total));
  int* hdr = reinterpret_cast<int*>(pack);
  double* dets = reinterpret_cast<double*>(pack + L.dets);
  int* ids = reinterpret_cast<int*>(pack + L.ids);
  const size_t wb = mscnn_detections_workspace_bytes(max_rows);
  void* ws = n->det_ws.Reserve(wb);
  const int words[4] = {S, R_all, cap, 0};
  MSCNN_CHECK(mscnn_store_words_i32(hdr, words, 4, st));
  for (int s = 0; s < S; ++s) {
    const int i = s / K, k = s % K, o = k / C;
    const SegSource& t = src[o];
    const int r0 = i > 0 ? end[o][i - 1] : 0, nr = end[o][i] - r0;
    const size_t slot = mscnn_multi_pack_slot(K, r0, k, nr);
    int* ent = hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s);
    const int e[3] = {nr, r0, 0};
    MSCNN_CHECK(mscnn_store_words_i32(ent + 1, e, 3, st));
    const float* boxes = t.boxes->gpu_data() + (size_t)r0 * (t.cascade ? 5 : 4 * t.ncls);
    const float* cls = t.cls->gpu_data() + (size_t)r0 * t.ncls;
    const float* props = t.props->gpu_data() + (size_t)r0 * (t.cascade ? 5 : 6);
    if (t.cascade) MSCNN_CHECK(mscnn_detections_cascade_nms_fwd(&desc[s], det_thr, nms, boxes, cls, props, nr, dets + 5 * slot, ids + slot, ent, ws, wb, st));
    else MSCNN_CHECK(mscnn_detections_nms_fwd(&desc[s], nms, boxes, cls, props, nr, dets + 5 * slot, ids + slot, ent, ws, wb, st));
  }
  *pack_out = pack;
  return false;
}

// The plain one-pass stage: everything that can be refused is refused here, then the one source and the descs go to segments_into_pack.
static bool detect_multi_into_pack(mscnn_net* n, const mscnn_detect_params* p, int num_images, int num_classes, int cap, char* pack_at,
                                   char** pack_out) {
  CHECK(p != nullptr);
  CHECK(num_images >= 1 && num_classes >= 1) << num_images << " images x " << num_classes << " classes";
  CHECK(n->net->has_blob("bbox_pred") && n->net->has_blob("cls_pred") && n->net->has_blob("proposals_score"))
      << "net has no bbox_pred / cls_pred / proposals_score outputs";
  const int num = n->net->num_inputs() > 0 && n->net->input_blobs()[0]->num_axes() == 4 ? n->net->input_blobs()[0]->num() : 1;
  CHECK_EQ(num_images, num) << "detect_multi: num_images " << num_images << " but the net's input holds " << num << " images";
  auto bbox = n->net->blob_by_name("bbox_pred");
  auto cls = n->net->blob_by_name("cls_pred");
  auto props = n->net->blob_by_name("proposals_score");
  const int R_all = props->num();
  CHECK_EQ(bbox->num(), R_all);
  CHECK_EQ(cls->num(), R_all);
  CHECK_GE(R_all, 1);
  const int ncls = cls->count() / R_all;
  CHECK_EQ(bbox->count() / R_all, 4 * ncls);
  CHECK_GE((long)cap, (long)num_classes * R_all) << "detection pack capacity " << cap << " < " << num_classes << " classes x " << R_all
                                                  << " ROIs (size it by BoxOutput's max_nms_num x images x classes)";
  const int S = num_images * num_classes;
  std::vector<mscnn_detections_desc> desc(S);
  for (int s = 0; s < S; ++s) {
    mscnn_detections_desc& d = desc[s];
    d.ncls = ncls;
    d.cls_id = p[s].cls_id;
    CHECK(d.cls_id >= 1 && d.cls_id <= ncls) << "segment " << s << ": cls_id " << d.cls_id << " of " << ncls;
    for (int k = 0; k < 4; ++k) { d.bbox_mean[k] = p[s].bbox_mean[k]; d.bbox_std[k] = p[s].bbox_std[k]; }
    d.proposal_thr = p[s].proposal_thr;
    d.ratio_h = p[s].ratio_h; d.ratio_w = p[s].ratio_w; d.org_h = p[s].org_h; d.org_w = p[s].org_w; d.nms_overlap = p[s].nms_overlap;
  }
  return segments_into_pack(n, {SegSource{bbox.get(), cls.get(), props.get(), ncls, false}}, desc, num_images, num_classes, 0.f, cap,
                            pack_at, pack_out);
}

// mscnn_net_render's record of the pack a blocking call has just left in det_host (ids: the tracker's ids lie at ids_at behind it)
static void render_keep(mscnn_net* n, int frames, int slots, int cap, bool ids, size_t ids_at) {
  mscnn_net::Render& r = n->render;
  r.frames = frames; r.slots = slots; r.cap = cap; r.ids = ids; r.ids_at = ids_at;
  r.bytes = ids ? ids_at + (size_t)(cap > 0 ? cap : 1) * sizeof(int) : mscnn_multi_pack_layout_of(frames * slots, cap).total;
  r.valid = true;
}

// The blocking form of both one-pass calls.  As mscnn_net_detect: the kernels write the pack straight into host-coherent pinned memory,
// one stream synchronisation, no copy; the per-segment fallback leaves it in the device pack and copies it.  rows_all: validates and
// returns R_all (the pack gets K R_all rows); into_pack(pack rows, pack_at, &pack): segments_into_pack's result.
static void detect_segments_blocking(mscnn_net* n, const char* name, int num_images, int K, const std::function<int()>& rows_all,
                                     const std::function<bool(int, char*, char**)>& into_pack, double* dets_host, int* ids_host, int cap,
                                     int* seg_dets, int* image_rois, bool tracked = false) {
  hipStream_t st = (hipStream_t)Caffe::stream();
  const int S = num_images * K;
  int pcap = 0;
  // the tracker (mscnn_net_set_tracker): the images are consecutive frames of the stream; the update runs behind the pack on the same
  // stream, its ids go behind the pack in the same pinned block and come over with it
  const bool track = tracked && n->track_on;
  if (tracked) n->tracks_valid = false;
  if (track) track_slots_checked(n, name, num_images, K);
  size_t ids_at = 0;
  auto run = [&]() {
    pcap = K * rows_all();
    const size_t total = mscnn_multi_pack_layout_of(S, pcap).total;
    ids_at = (total + 15) / 16 * 16;
    ensure_det_host(n, track ? ids_at + (size_t)(pcap > 0 ? pcap : 1) * sizeof(int) : total);
    *static_cast<volatile int*>(n->det_host) = -1;      // the header's first word (S): the kernels must have written it
    char* pack = nullptr;
    const bool there = into_pack(pcap, static_cast<char*>(n->det_host_dev), &pack);
    if (track) track_enqueue(n, name, num_images, K, pack, pcap, reinterpret_cast<int*>(static_cast<char*>(n->det_host_dev) + ids_at));
    if (!there) HIP_CHECK(hipMemcpyAsync(n->det_host, pack, total, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  };
  run();
  if (n->net->HandoffRecover()) run();      // (as mscnn_net_detect: the frame has been run again on whole tiles)
  const int* hdr = static_cast<const int*>(n->det_host);
  CHECK_GE(hdr[0], 0) << name << ": the pack header was not written (" << S << " segments, " << pcap << " pack rows)";
  for (int s = 0; s < S; ++s) {
    const int count = hdr[MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s)];
    CHECK_GE(count, -1) << name << ": segment " << s << " has count " << count;
  }
  const int rc = mscnn_net_unpack_detections_multi(n->det_host, num_images, K, pcap, dets_host, ids_host, cap, seg_dets, image_rois);
  CHECK_EQ(rc, 0) << g_err;
  if (track) {      // the call has succeeded: commit the table, keep the ids of the detections just returned, in their order
    track_commit(n, K);
    const int* th = reinterpret_cast<const int*>(static_cast<const char*>(n->det_host) + ids_at);
    n->track_ids.clear();
    for (int s = 0; s < S; ++s) {
      const int* e = hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s);
      const size_t slot = mscnn_multi_pack_slot(K, e[2], s % K, e[1]);
      n->track_ids.insert(n->track_ids.end(), th + slot, th + slot + seg_dets[s]);
    }
    n->track_seg_dets.assign(seg_dets, seg_dets + S);
    n->tracks_valid = true;
  }
  if (tracked) render_keep(n, num_images, K, pcap, track, ids_at);
}

size_t mscnn_net_detect_multi_pack_bytes(int num_images, int num_classes, int cap) {
  return mscnn_detections_multi_pack_bytes(num_images * num_classes, cap);
}

int mscnn_net_detect_multi_device(mscnn_net* n, const mscnn_detect_params* p, int num_images, int num_classes, int cap,
                                  const void** pack_dev) {
  return guarded([&] {
    CHECK(pack_dev != nullptr);
    track_refuses(n, "detect_multi_device");
    char* pack = nullptr;
    detect_multi_into_pack(n, p, num_images, num_classes, cap, nullptr, &pack);
    *pack_dev = pack;
  });
}

int mscnn_net_unpack_detections_multi(const void* pack_host, int num_images, int num_classes, int cap, double* dets_host, int* ids_host,
                                      int out_cap, int* seg_dets, int* image_rois) {
  return guarded([&] {
    CHECK(pack_host && seg_dets) << "unpack_detections_multi: null pointer";
    CHECK(num_images >= 1 && num_classes >= 1) << num_images << " images x " << num_classes << " classes";
    const int S = num_images * num_classes;
    const char* hp = static_cast<const char*>(pack_host);
    const int* hdr = reinterpret_cast<const int*>(hp);
    CHECK_EQ(hdr[0], S) << "detection pack was written for another number of segments";
    CHECK_EQ(hdr[2], cap) << "detection pack was written for another capacity";
    const int R_all = hdr[1];
    CHECK(R_all >= 0 && (long)num_classes * R_all <= (long)cap && hdr[3] == 0)
        << "corrupt detection pack header: " << R_all << " ROIs, capacity " << cap;
    long D = 0;
    for (int s = 0; s < S; ++s) {
      const int* e = hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s);
      const int i = s / num_classes;
      CHECK(e[0] != -1) << "image " << i << " has " << e[1] << " ROIs, more than the per-image row bound the stage was sized by";
      CHECK(e[0] >= 0 && e[0] <= e[1] && e[2] >= 0 && (long)e[2] + e[1] <= R_all && e[3] == 0)
          << "corrupt detection pack: segment " << s << " has " << e[0] << " detections, rows [" << e[2] << ", +" << e[1] << ") of " << R_all;
      const int* e0 = hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + i * num_classes);
      CHECK(e[1] == e0[1] && e[2] == e0[2]) << "corrupt detection pack: the segments of image " << i << " disagree on its rows";
      D += e[0];
    }
    CHECK_LE(D, (long)out_cap) << "detections buffer holds " << out_cap << " rows, the " << S << " segments have " << D;
    CHECK(D == 0 || dets_host) << "unpack_detections_multi: null dets buffer";
    const mscnn_multi_pack_layout L = mscnn_multi_pack_layout_of(S, cap);
    const double* pd = reinterpret_cast<const double*>(hp + L.dets);
    const int* pi = reinterpret_cast<const int*>(hp + L.ids);
    size_t o = 0;
    for (int s = 0; s < S; ++s) {
      const int* e = hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s);
      const int c = s % num_classes, cnt = e[0], rows = e[1], row0 = e[2];
      const size_t slot = mscnn_multi_pack_slot(num_classes, row0, c, rows);
      if (cnt > 0) std::memcpy(dets_host + 5 * o, pd + 5 * slot, sizeof(double) * 5 * cnt);
      if (cnt > 0 && ids_host)
        for (int k = 0; k < cnt; ++k) ids_host[o + k] = pi[slot + k] + row0;      // rows of the net's ROI blobs, as detect_image
      seg_dets[s] = cnt;
      if (image_rois && c == 0) image_rois[s / num_classes] = rows;
      o += cnt;
    }
  });
}

int mscnn_net_detect_multi(mscnn_net* n, const mscnn_detect_params* p, int num_images, int num_classes, double* dets_host, int* ids_host,
                           int cap, int* seg_dets, int* image_rois) {
  return guarded([&] {
    CHECK(p && seg_dets) << "detect_multi: null pointer";
    CHECK(num_images >= 1 && num_classes >= 1) << num_images << " images x " << num_classes << " classes";
    detect_segments_blocking(
        n, "detect_multi", num_images, num_classes,
        [&] {
          CHECK(n->net->has_blob("proposals_score")) << "net has no proposals_score output";
          return n->net->blob_by_name("proposals_score")->num();
        },
        [&](int pcap, char* pack_at, char** pack) { return detect_multi_into_pack(n, p, num_images, num_classes, pcap, pack_at, pack); },
        dets_host, ids_host, cap, seg_dets, image_rois, true);
  });
}

// The nets whose drivers have a proposal result: a proposals_score blob, and no cascade stage behind it.  (The cascade deploys carry
// the blob too -- their BoxOutput is the plain nets' --, but run_cascademscnn.m never reads it: proposals for the cascade outputs are
// not restated, so a net with a DecodeBBox layer is refused by that layer's name instead of being answered with the first stage's.)
static int proposals_rows_checked(const mscnn_net* n) {
  CHECK(n->net->has_blob("proposals_score")) << "net has no proposals_score blob: nothing to take the proposals from";
  const auto& layers = n->net->layers();
  for (size_t l = 0; l < layers.size(); ++l)
    CHECK(std::strcmp(layers[l]->type(), "DecodeBBox") != 0)
        << "net is a cascade deploy (DecodeBBox layer " << n->net->layer_names()[l] << "): the cascade drivers output no proposals, "
        << "its proposals_score is not restated";
  return n->net->blob_by_name("proposals_score")->num();
}

// The proposal result of the last forward (mscnn_hip.h: mscnn_proposals_multi_fwd) into the multi pack with one slot per image, at
// pack_at (device-addressable) or in the net's device pack.  Everything that can be refused is refused before the launch.
static bool proposals_into_pack(mscnn_net* n, const mscnn_detect_params* p, int num_images, int cap, char* pack_at, char** pack_out) {
  CHECK(p != nullptr) << "proposals_multi: null params";
  CHECK_GE(num_images, 1) << "proposals_multi: " << num_images << " images";
  proposals_rows_checked(n);
  const int num = n->net->num_inputs() > 0 && n->net->input_blobs()[0]->num_axes() == 4 ? n->net->input_blobs()[0]->num() : 1;
  CHECK_EQ(num_images, num) << "proposals_multi: num_images " << num_images << " but the net's input holds " << num << " images";
  auto props = n->net->blob_by_name("proposals_score");
  const int R_all = props->num();
  CHECK_GE(R_all, 1) << "proposals_score has no rows: no forward has run";
  CHECK_EQ(props->count() / R_all, 6) << "proposals_score rows are [img x1 y1 x2 y2 score]";
  CHECK_GE(cap, R_all) << "proposal pack capacity " << cap << " < " << R_all << " ROIs (size it by BoxOutput's max_nms_num x images)";
  std::vector<mscnn_proposals_desc> desc(num_images);
  for (int i = 0; i < num_images; ++i) desc[i] = mscnn_proposals_desc{p[i].proposal_thr, p[i].ratio_h, p[i].ratio_w};
  char* pack = pack_at ? pack_at : static_cast<char*>(n->det_pack.Reserve(mscnn_multi_pack_layout_of(num_images, cap).total));
  MSCNN_CHECK(mscnn_proposals_multi_fwd(desc.data(), num_images, props->gpu_data(), R_all, pack, cap, Caffe::stream()));
  *pack_out = pack;
  return pack == pack_at;
}

int mscnn_net_proposals_multi(mscnn_net* n, const mscnn_detect_params* p, int num_images, double* props_host, int* rows_host, int cap,
                              int* image_props, int* image_rois) {
  return guarded([&] {
    CHECK(p && image_props) << "proposals_multi: null pointer";
    CHECK_GE(num_images, 1) << "proposals_multi: " << num_images << " images";
    detect_segments_blocking(
        n, "proposals_multi", num_images, 1,
        [&] { return proposals_rows_checked(n); },
        [&](int pcap, char* pack_at, char** pack) { return proposals_into_pack(n, p, num_images, pcap, pack_at, pack); }, props_host,
        rows_host, cap, image_props, image_rois);
  });
}

int mscnn_net_proposals_multi_device(mscnn_net* n, const mscnn_detect_params* p, int num_images, int cap, const void** pack_dev) {
  return guarded([&] {
    CHECK(pack_dev != nullptr);
    char* pack = nullptr;
    proposals_into_pack(n, p, num_images, cap, nullptr, &pack);
    *pack_dev = pack;
  });
}

int mscnn_net_forward_proposals(mscnn_net* n, int* last_layer) {
  return guarded([&] {
    int L = -1;
    const auto& layers = n->net->layers();
    const Blob<float>* want = n->net->has_blob("proposals_score") ? n->net->blob_by_name("proposals_score").get() : nullptr;
    for (size_t l = 0; l < layers.size() && L < 0 && want; ++l)
      if (std::strcmp(layers[l]->type(), "BoxOutput") == 0 && n->net->top_vecs()[l].size() >= 2 && n->net->top_vecs()[l][1] == want)
        L = (int)l;
    CHECK_GE(L, 0) << "net has no BoxOutput layer whose second top is proposals_score";
    // (a range that ends in front of the sub-net: BoxOutput's before-sync hook sees last_end_ < its convolution and builds no ROI
    // maps, and `whole` is false for the numerics watch -- Net::ForwardFromTo)
    n->net->ForwardFromTo(0, L);
    if (last_layer) *last_layer = L;
  });
}

int mscnn_net_forward_rois_layers(const mscnn_net* n, int* L, int* K) {
  return guarded([&] {
    CHECK(n && L && K) << "forward_rois_layers: null pointer";
    n->net->RoisLayers(L, K);
    CHECK_GE(*L, 0) << "forward_rois: net has no ROIPooling / ROIAlign layer fed by a BoxOutput layer: nothing to run on caller-supplied ROIs";
  });
}

int mscnn_net_forward_rois(mscnn_net* n, const void* rows, int on_device, int coords, int R, const mscnn_detect_params* p, int num_images,
                           int run_trunk, int* image_rois) {
  return guarded([&] {
    CHECK(n != nullptr) << "forward_rois: null net";
    CHECK_GE(n->device, 0) << "forward_rois: the net was built with device " << n->device << " (graph only): nothing can run";
    CHECK(rows != nullptr) << "forward_rois: null rows";
    CHECK_GE(num_images, 1) << "forward_rois: num_images = " << num_images;
    CHECK(coords == MSCNN_ROIS_NET || p != nullptr) << "forward_rois: original-image coordinates need params (num_images of them: "
                                                       "ratio_h, ratio_w)";
    std::vector<double> rh, rw;
    if (coords != MSCNN_ROIS_NET && p)
      for (int i = 0; i < num_images; ++i) { rh.push_back(p[i].ratio_h); rw.push_back(p[i].ratio_w); }
    n->net->ForwardRois(rows, on_device != 0, coords, R, rh.empty() ? nullptr : rh.data(), rw.empty() ? nullptr : rw.data(), num_images,
                        run_trunk != 0, image_rois);
  });
}

int mscnn_net_reshape_input(mscnn_net* n, const char* name, const int* dims, int ndim) {
  return guarded([&] {
    CHECK(n->net->has_blob(name)) << "Unknown blob name " << name;
    CHECK(dims && ndim >= 1 && ndim <= 8);
    bool is_input = false;
    for (int i = 0; i < n->net->num_inputs(); ++i)
      is_input = is_input || n->net->blob_names()[n->net->input_blob_indices()[i]] == name;
    CHECK(is_input) << "blob " << name << " is not a net input";
    n->net->MaterializePendingReadersOf(name);
    n->net->MaterializeStale();      // (blobs the last forward left unwritten belong to the OLD shape)
    std::vector<int> shape(dims, dims + ndim);
    n->net->blob_by_name(name)->Reshape(shape);      // blob->Reshape + net->Reshape: matcaffe's net.blobs('data').reshape(..); net.reshape()
    n->net->Reshape();
  });
}

int mscnn_net_detect_cascade(mscnn_net* n, const mscnn_detect_params* p, float det_thr, const char* bbox_blob, const char* prob_blob,
                             const char* proposal_blob, double* dets_host, int* ids_host, int cap, int* num_dets, int* num_rois) {
  return guarded([&] {
    CHECK(p && dets_host && num_dets && bbox_blob && prob_blob && proposal_blob);
    track_refuses(n, "detect_cascade");
    for (const char* b : {bbox_blob, prob_blob, proposal_blob}) CHECK(n->net->has_blob(b)) << "Unknown blob name " << b;
    auto boxes = n->net->blob_by_name(bbox_blob);
    auto prob = n->net->blob_by_name(prob_blob);
    auto props = n->net->blob_by_name(proposal_blob);
    const int R = boxes->num();
    CHECK_EQ(prob->num(), R);
    CHECK_EQ(props->num(), R);
    CHECK_EQ(boxes->count(), 5 * R) << bbox_blob << " is not an [R, 5] box blob";
    mscnn_detections_desc d;
    std::memset(&d, 0, sizeof(d));
    d.ncls = R > 0 ? prob->count() / R : 1;
    d.cls_id = p->cls_id;
    d.ratio_h = p->ratio_h; d.ratio_w = p->ratio_w; d.org_h = p->org_h; d.org_w = p->org_w; d.nms_overlap = p->nms_overlap;
    const size_t wb = mscnn_detections_workspace_bytes(R);
    void* ws = n->det_ws.Reserve(wb);
    const size_t rows = (size_t)(R > 0 ? R : 1), total = mscnn_net_detect_pack_bytes((int)rows);
    char* pack = static_cast<char*>(n->det_pack.Reserve(total));
    hipStream_t st = (hipStream_t)Caffe::stream();
    MSCNN_CHECK(mscnn_detections_cascade_nms_fwd(&d, det_thr, nms_arg(n, true), boxes->gpu_data(), prob->gpu_data(), props->gpu_data(), R,
                                                 reinterpret_cast<double*>(pack + 16), reinterpret_cast<int*>(pack + 16 + sizeof(double) * 5 * rows),
                                                 reinterpret_cast<int*>(pack), ws, wb, st));
    ensure_det_host(n, total);
    HIP_CHECK(hipMemcpyAsync(n->det_host, pack, total, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const char* hp = static_cast<const char*>(n->det_host);
    const int D = *reinterpret_cast<const int*>(hp);
    CHECK_LE(D, cap) << "detections buffer too small";
    if (D > 0) {
      std::memcpy(dets_host, hp + 16, sizeof(double) * 5 * D);
      if (ids_host) std::memcpy(ids_host, hp + 16 + sizeof(double) * 5 * rows, sizeof(int) * D);
    }
    *num_dets = D;
    if (num_rois) *num_rois = R;
  });
}

// ---- every (image, cascade output, class) segment of the last forward in one pass ------------------------------------------------------
// The blob triples of the cascade outputs, checked: names, [R, 5] boxes and proposals, one row count throughout.
struct CascadeBlobs {
  std::vector<SegSource> src;
  int R_all = 0;
};
static CascadeBlobs cascade_blobs(mscnn_net* n, int num_outputs, const char* const* bbox_blobs, const char* const* prob_blobs,
                                  const char* const* proposal_blobs) {
  CHECK(num_outputs >= 1 && num_outputs <= 4) << "detect_cascade_multi: " << num_outputs << " cascade outputs (1 .. 4)";
  CHECK(bbox_blobs && prob_blobs && proposal_blobs) << "detect_cascade_multi: null blob name list";
  CascadeBlobs b;
  for (int o = 0; o < num_outputs; ++o) {
    CHECK(bbox_blobs[o] && prob_blobs[o] && proposal_blobs[o]) << "detect_cascade_multi: output " << o << " of " << num_outputs
                                                               << ": null blob name";
    for (const char* name : {bbox_blobs[o], prob_blobs[o], proposal_blobs[o]})
      CHECK(n->net->has_blob(name)) << "Unknown blob name " << name << " (cascade output " << o << ")";
    const Blob<float>* boxes = n->net->blob_by_name(bbox_blobs[o]).get();
    const Blob<float>* prob = n->net->blob_by_name(prob_blobs[o]).get();
    const Blob<float>* props = n->net->blob_by_name(proposal_blobs[o]).get();
    const int R = boxes->num();
    CHECK(prob->num() == R && props->num() == R) << "cascade output " << o << ": " << bbox_blobs[o] << " has " << R << " rows, "
                                                 << prob_blobs[o] << " " << prob->num() << ", " << proposal_blobs[o] << " " << props->num();
    if (o == 0) b.R_all = R;
    CHECK_EQ(R, b.R_all) << "cascade output " << o << " has " << R << " rows, output 0 has " << b.R_all;
    CHECK_GE(R, 1) << "cascade output " << o << " has no rows";
    CHECK_EQ(boxes->count(), 5 * R) << bbox_blobs[o] << " is not an [R, 5] box blob (" << boxes->count() << " values in " << R << " rows)";
    CHECK_EQ(props->count(), 5 * R) << proposal_blobs[o] << " is not an [R, 5] proposal blob (" << props->count() << " values in " << R
                                    << " rows)";
    b.src.push_back(SegSource{boxes, prob, props, prob->count() / R, true});
  }
  return b;
}

// Everything that can be refused is refused here, before any device memory is reserved or a kernel launched.  Returns the descs.
static std::vector<mscnn_detections_desc> cascade_descs(mscnn_net* n, const mscnn_detect_params* p, int num_images, int num_outputs,
                                                        int num_classes, const CascadeBlobs& b, int cap) {
  CHECK(p != nullptr) << "detect_cascade_multi: null pointer";
  CHECK(num_images >= 1 && num_classes >= 1) << num_images << " images x " << num_classes << " classes";
  const int num = n->net->num_inputs() > 0 && n->net->input_blobs()[0]->num_axes() == 4 ? n->net->input_blobs()[0]->num() : 1;
  CHECK_EQ(num_images, num) << "detect_cascade_multi: num_images " << num_images << " but the net's input holds " << num << " images";
  const int K = num_outputs * num_classes, S = num_images * K;
  CHECK_GE((long)cap, (long)K * b.R_all) << "detection pack capacity " << cap << " < " << num_outputs << " outputs x " << num_classes
                                         << " classes x " << b.R_all << " ROIs";
  std::vector<mscnn_detections_desc> desc(S);
  for (int s = 0; s < S; ++s) {
    const int o = (s % K) / num_classes;
    mscnn_detections_desc& d = desc[s];
    std::memset(&d, 0, sizeof(d));
    d.ncls = b.src[o].ncls;
    d.cls_id = p[s].cls_id;
    CHECK(d.cls_id >= 1 && d.cls_id <= d.ncls) << "segment " << s << " (output " << o << "): cls_id " << d.cls_id << " of " << d.ncls;
    d.ratio_h = p[s].ratio_h; d.ratio_w = p[s].ratio_w; d.org_h = p[s].org_h; d.org_w = p[s].org_w; d.nms_overlap = p[s].nms_overlap;
  }
  return desc;
}

size_t mscnn_net_detect_cascade_multi_pack_bytes(int num_images, int num_outputs, int num_classes, int cap) {
  return mscnn_detections_multi_pack_bytes(num_images * num_outputs * num_classes, cap);
}

int mscnn_net_detect_cascade_multi_device(mscnn_net* n, const mscnn_detect_params* p, int num_images, int num_outputs, int num_classes,
                                          const char* const* bbox_blobs, const char* const* prob_blobs, const char* const* proposal_blobs,
                                          float det_thr, int cap, const void** pack_dev) {
  return guarded([&] {
    CHECK(pack_dev != nullptr) << "detect_cascade_multi_device: null pointer";
    track_refuses(n, "detect_cascade_multi_device");
    const CascadeBlobs b = cascade_blobs(n, num_outputs, bbox_blobs, prob_blobs, proposal_blobs);
    const auto desc = cascade_descs(n, p, num_images, num_outputs, num_classes, b, cap);
    char* pack = nullptr;
    segments_into_pack(n, b.src, desc, num_images, num_classes, det_thr, cap, nullptr, &pack);
    *pack_dev = pack;
  });
}

int mscnn_net_detect_cascade_multi(mscnn_net* n, const mscnn_detect_params* p, int num_images, int num_outputs, int num_classes,
                                   const char* const* bbox_blobs, const char* const* prob_blobs, const char* const* proposal_blobs,
                                   float det_thr, double* dets_host, int* ids_host, int cap, int* seg_dets, int* image_rois) {
  return guarded([&] {
    CHECK(p && seg_dets) << "detect_cascade_multi: null pointer";
    CascadeBlobs b;
    std::vector<mscnn_detections_desc> desc;
    detect_segments_blocking(
        n, "detect_cascade_multi", num_images, num_outputs * num_classes,
        [&] {
          b = cascade_blobs(n, num_outputs, bbox_blobs, prob_blobs, proposal_blobs);
          desc = cascade_descs(n, p, num_images, num_outputs, num_classes, b, num_outputs * num_classes * b.R_all);
          return b.R_all;
        },
        [&](int pcap, char* pack_at, char** pack) { return segments_into_pack(n, b.src, desc, num_images, num_classes, det_thr, pcap, pack_at, pack); },
        dets_host, ids_host, cap, seg_dets, image_rois, true);
  });
}

// ---- several forwards of an image, one NMS (mscnn_hip.h: mscnn_detections_candidates_*, mscnn_detections_merge_fwd) -------------------
int mscnn_net_detect_merge_begin(mscnn_net* n, int num_images, int num_classes, int cand_cap) {
  return guarded([&] {
    mscnn_net::Merge& m = n->merge;
    CHECK(!m.open) << "detect_merge_begin: a merge of " << m.images << " images x " << m.slots << " slots with " << m.passes
                   << " forwards added is open (call mscnn_net_detect_merge_end first)";
    CHECK(num_images >= 1 && num_classes >= 1) << "detect_merge_begin: " << num_images << " images x " << num_classes << " classes";
    CHECK_GE(cand_cap, 1) << "detect_merge_begin: cand_cap " << cand_cap;
    // (while Seq-NMS is on the lists are the frames of a clip: what the op would refuse at _end is refused here, and nothing is opened)
    CHECK(n->seq.link_thr == 0.0 || num_images <= 256) << "detect_merge_begin: num_frames " << num_images << " is outside [1, 256] while Seq-NMS is on "
                                                          "(set_seq_nms link_thr " << n->seq.link_thr << ")";
    const int S = num_images * num_classes;
    const size_t bytes = mscnn_detections_candidates_bytes(S, cand_cap);
    CHECK_GT(bytes, 0u) << "detect_merge_begin: " << S << " segments x " << cand_cap << " candidate slots";
    CHECK_GE(n->device, 0) << "detect_merge_begin: the net was built with device " << n->device << " (graph only): no candidate lists";
    MSCNN_CHECK(mscnn_detections_candidates_reset(m.cand.Reserve(bytes), S, cand_cap, Caffe::stream()));
    m.open = true; m.images = num_images; m.slots = num_classes; m.cand_cap = cand_cap; m.passes = 0; m.rows = 0;
    m.handoff_errors = n->net->handoff_errors();
    m.overlap.assign(S, 0.5);      // (a list no add ever reaches stays empty: its overlap is never applied)
    m.overlap_known.assign(S, 0);
    m.views.assign(num_images, 0);
  });
}

// What the add calls check alike before anything is enqueued; R_all = the rows of this forward's ROI blobs.  list_of (NULL: image i
// is list i): the lists of which frame each of the num_images images of this forward goes to.
static void merge_add_checked(mscnn_net* n, const char* name, const mscnn_detect_params* p, int num_images, int slots, int R_all,
                              const int* list_of = nullptr) {
  mscnn_net::Merge& m = n->merge;
  CHECK(p != nullptr) << name << ": null params";
  CHECK_EQ(slots, m.slots) << name << ": " << slots << " slots per image, the merge was begun with " << m.slots;
  CHECK_LT(m.passes, 128) << name << ": " << m.passes << " forwards have been added, the tag holds 7 bits of pass";
  CHECK_LE(m.rows + R_all, (long)m.cand_cap) << name << ": the " << m.passes << " forwards added so far have " << m.rows
                                             << " ROI rows, this one " << R_all << ": more than cand_cap " << m.cand_cap;
  const int S = num_images * slots;
  std::vector<double> seen(m.overlap);
  std::vector<char> known(m.overlap_known);
  for (int s = 0; s < S; ++s) {
    CHECK(!(p[s].nms_overlap != p[s].nms_overlap)) << name << ": segment " << s << ": nms_overlap is NaN";
    const int l = (list_of ? list_of[s / slots] : s / slots) * slots + s % slots;
    if (known[l])
      CHECK(p[s].nms_overlap == seen[l]) << name << ": segment " << s << ": nms_overlap " << p[s].nms_overlap
                                         << (m.overlap_known[l] ? ", the first forward of this merge was added with " : ", an image of this forward in front of it goes to the same list with ")
                                         << seen[l];
    seen[l] = p[s].nms_overlap; known[l] = 1;
  }
}
static void merge_added(mscnn_net* n, const mscnn_detect_params* p, int S, int R_all, const int* list_of = nullptr) {
  mscnn_net::Merge& m = n->merge;
  for (int s = 0; s < S; ++s) {
    const int l = (list_of ? list_of[s / m.slots] : s / m.slots) * m.slots + s % m.slots;
    if (!m.overlap_known[l]) { m.overlap[l] = p[s].nms_overlap; m.overlap_known[l] = 1; }
  }
  for (int b = 0; b < S / m.slots; ++b) ++m.views[list_of ? list_of[b] : b];
  ++m.passes;
  m.rows += R_all;
}
// list_of of the views adds: one entry per image of the input, each a frame of the open merge
static void merge_list_of_checked(mscnn_net* n, const char* name, const int* list_of, int num_images) {
  CHECK(list_of != nullptr) << name << ": null list_of";
  for (int b = 0; b < num_images; ++b)
    CHECK(list_of[b] >= 0 && list_of[b] < n->merge.images) << name << ": image " << b << ": list_of " << list_of[b] << " outside [0, "
                                                           << n->merge.images << "): the merge was begun with " << n->merge.images << " frames";
}
static int merge_input_images(mscnn_net* n) {
  return n->net->num_inputs() > 0 && n->net->input_blobs()[0]->num_axes() == 4 ? n->net->input_blobs()[0]->num() : 1;
}

// the plain add (list_of NULL: the merge's images are the input's) and its views form (any N, image b to the lists of frame list_of[b])
static void merge_add_plain(mscnn_net* n, const char* name, const mscnn_detect_params* p, const mscnn_detections_view* view, bool views,
                            const int* list_of) {
  const std::string nm(name);
  mscnn_net::Merge& m = n->merge;
  CHECK(m.open) << nm << ": no merge is open (call mscnn_net_detect_merge_begin first)";
  const int num = merge_input_images(n);
  if (views) merge_list_of_checked(n, name, list_of, num);
  else CHECK_EQ(m.images, num) << nm << ": the merge was begun with " << m.images << " images but the net's input holds " << num;
  CHECK(n->net->has_blob("bbox_pred") && n->net->has_blob("cls_pred") && n->net->has_blob("proposals_score"))
      << nm << ": net has no bbox_pred / cls_pred / proposals_score outputs";
  auto bbox = n->net->blob_by_name("bbox_pred");
  auto cls = n->net->blob_by_name("cls_pred");
  auto props = n->net->blob_by_name("proposals_score");
  const int R_all = props->num();
  CHECK_GE(R_all, 1);
  CHECK(bbox->num() == R_all && cls->num() == R_all) << nm << ": bbox_pred has " << bbox->num() << " rows, cls_pred " << cls->num()
                                                      << ", proposals_score " << R_all;
  const int ncls = cls->count() / R_all;
  CHECK_EQ(bbox->count() / R_all, 4 * ncls);
  merge_add_checked(n, name, p, num, m.slots, R_all, list_of);
  const int S = num * m.slots;
  std::vector<mscnn_detections_desc> desc(S);
  for (int s = 0; s < S; ++s) {
    mscnn_detections_desc& d = desc[s];
    d.ncls = ncls;
    d.cls_id = p[s].cls_id;
    CHECK(d.cls_id >= 1 && d.cls_id <= ncls) << nm << ": segment " << s << ": cls_id " << d.cls_id << " of " << ncls;
    for (int k = 0; k < 4; ++k) { d.bbox_mean[k] = p[s].bbox_mean[k]; d.bbox_std[k] = p[s].bbox_std[k]; }
    d.proposal_thr = p[s].proposal_thr;
    d.ratio_h = p[s].ratio_h; d.ratio_w = p[s].ratio_w; d.org_h = p[s].org_h; d.org_w = p[s].org_w; d.nms_overlap = p[s].nms_overlap;
  }
  if (list_of)
    MSCNN_CHECK(mscnn_detections_candidates_add_views(desc.data(), view, list_of, nms_arg(n, false), m.passes, num, m.images, m.slots,
                                                      bbox->gpu_data(), cls->gpu_data(), props->gpu_data(), R_all, m.cand.get(), m.cand_cap,
                                                      Caffe::stream()));
  else
    MSCNN_CHECK(mscnn_detections_candidates_add(desc.data(), view, nms_arg(n, false), m.passes, m.images, m.slots, bbox->gpu_data(),
                                                cls->gpu_data(), props->gpu_data(), R_all, m.cand.get(), m.cand_cap, Caffe::stream()));
  merge_added(n, p, S, R_all, list_of);
}

int mscnn_net_detect_merge_add(mscnn_net* n, const mscnn_detect_params* p, const mscnn_detections_view* view) {
  return guarded([&] { merge_add_plain(n, "detect_merge_add", p, view, false, nullptr); });
}
int mscnn_net_detect_merge_add_views(mscnn_net* n, const mscnn_detect_params* p, const mscnn_detections_view* view, const int* list_of) {
  return guarded([&] { merge_add_plain(n, "detect_merge_add_views", p, view, true, list_of); });
}

static void merge_add_cascade(mscnn_net* n, const char* name, const mscnn_detect_params* p, const mscnn_detections_view* view,
                              bool views, const int* list_of, int num_outputs, const char* const* bbox_blobs,
                              const char* const* prob_blobs, const char* const* proposal_blobs, float det_thr) {
  const std::string nm(name);
  mscnn_net::Merge& m = n->merge;
  CHECK(m.open) << nm << ": no merge is open (call mscnn_net_detect_merge_begin first)";
  const int num = merge_input_images(n);
  if (views) merge_list_of_checked(n, name, list_of, num);
  else CHECK_EQ(m.images, num) << nm << ": the merge was begun with " << m.images << " images but the net's input holds " << num;
  const CascadeBlobs b = cascade_blobs(n, num_outputs, bbox_blobs, prob_blobs, proposal_blobs);
  CHECK_EQ(m.slots % num_outputs, 0) << nm << ": the merge was begun with " << m.slots << " slots per image, not a multiple of "
                                     << num_outputs << " cascade outputs";
  const int C = m.slots / num_outputs;
  merge_add_checked(n, name, p, num, m.slots, b.R_all, list_of);
  const int S = num * m.slots;
  const auto desc = cascade_descs(n, p, num, num_outputs, C, b, m.slots * b.R_all);
  std::vector<mscnn_cascade_output> outs(num_outputs);
  for (int o = 0; o < num_outputs; ++o)
    outs[o] = mscnn_cascade_output{b.src[o].boxes->gpu_data(), b.src[o].cls->gpu_data(), b.src[o].props->gpu_data(), b.src[o].ncls};
  if (list_of)
    MSCNN_CHECK(mscnn_detections_candidates_cascade_add_views(desc.data(), view, list_of, det_thr, nms_arg(n, true), m.passes, num, m.images,
                                                              num_outputs, C, outs.data(), b.R_all, m.cand.get(), m.cand_cap, Caffe::stream()));
  else
    MSCNN_CHECK(mscnn_detections_candidates_cascade_add(desc.data(), view, det_thr, nms_arg(n, true), m.passes, m.images, num_outputs, C,
                                                        outs.data(), b.R_all, m.cand.get(), m.cand_cap, Caffe::stream()));
  merge_added(n, p, S, b.R_all, list_of);
}

int mscnn_net_detect_cascade_merge_add(mscnn_net* n, const mscnn_detect_params* p, const mscnn_detections_view* view, int num_outputs,
                                       const char* const* bbox_blobs, const char* const* prob_blobs, const char* const* proposal_blobs,
                                       float det_thr) {
  return guarded([&] { merge_add_cascade(n, "detect_cascade_merge_add", p, view, false, nullptr, num_outputs, bbox_blobs, prob_blobs, proposal_blobs, det_thr); });
}
int mscnn_net_detect_cascade_merge_add_views(mscnn_net* n, const mscnn_detect_params* p, const mscnn_detections_view* view, const int* list_of,
                                             int num_outputs, const char* const* bbox_blobs, const char* const* prob_blobs,
                                             const char* const* proposal_blobs, float det_thr) {
  return guarded([&] {
    merge_add_cascade(n, "detect_cascade_merge_add_views", p, view, true, list_of, num_outputs, bbox_blobs, prob_blobs, proposal_blobs, det_thr);
  });
}

// The merge pack on the host -> segment after segment; the int column is a tag (pass << 24 | row), which mscnn_net_unpack_detections_multi
// would take for an id relative to row0: this pack has its own reader.
static void unpack_merge(const void* pack_host, int S, int cand_cap, double* dets_host, int* pass_host, int* row_host, int out_cap,
                         int* seg_dets, int* seg_candidates) {
  const char* hp = static_cast<const char*>(pack_host);
  const int* hdr = reinterpret_cast<const int*>(hp);
  CHECK(hdr[0] == S && hdr[1] == cand_cap && hdr[2] == S * cand_cap && hdr[3] == 0)
      << "detect_merge_end: the pack header was not written or is another merge's: {" << hdr[0] << ", " << hdr[1] << ", " << hdr[2] << ", "
      << hdr[3] << "} for " << S << " segments x " << cand_cap << " slots";
  long D = 0;
  for (int s = 0; s < S; ++s) {
    const int* e = hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s);
    CHECK(e[0] != -1) << "detect_merge_end: segment " << s << ": " << e[1] << " candidates wanted into a list of " << cand_cap << " slots";
    CHECK(e[0] >= 0 && e[0] <= e[1] && e[1] <= cand_cap && e[2] == s * cand_cap && e[3] == 0)
        << "corrupt merge pack: segment " << s << " has " << e[0] << " detections of " << e[1] << " candidates at row " << e[2];
    D += e[0];
  }
  CHECK_LE(D, (long)out_cap) << "detect_merge_end: detections buffer holds " << out_cap << " rows, the " << S << " segments have " << D;
  CHECK(D == 0 || dets_host) << "detect_merge_end: null dets buffer";
  const mscnn_multi_pack_layout L = mscnn_multi_pack_layout_of(S, S * cand_cap);
  const double* pd = reinterpret_cast<const double*>(hp + L.dets);
  const int* pi = reinterpret_cast<const int*>(hp + L.ids);
  size_t o = 0;
  for (int s = 0; s < S; ++s) {
    const int* e = hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + s);
    const int cnt = e[0];
    const size_t slot = (size_t)e[2];
    if (cnt > 0) std::memcpy(dets_host + 5 * o, pd + 5 * slot, sizeof(double) * 5 * cnt);
    for (int k = 0; k < cnt; ++k) {
      const int tag = pi[slot + k];
      if (pass_host) pass_host[o + k] = tag >> 24;
      if (row_host) row_host[o + k] = tag & 0xffffff;
    }
    seg_dets[s] = cnt;
    if (seg_candidates) seg_candidates[s] = e[1];
    o += cnt;
  }
}

int mscnn_net_detect_merge_end(mscnn_net* n, double* dets_host, int* pass_host, int* row_host, int cap, int* seg_dets, int* seg_candidates) {
  return guarded([&] {
    mscnn_net::Merge& m = n->merge;
    n->sequences_valid = false;      // (whatever happens from here on: detect_merge_sequences answers for THIS _end only)
    n->tracks_valid = false;         // (and detect_tracks)
    CHECK(m.open) << "detect_merge_end: no merge is open (call mscnn_net_detect_merge_begin first)";
    m.open = false;      // (whatever happens from here on: the merge is closed)
    // (the setting may have been turned on behind _begin: the op's own refusal of the shape, made here so that it names the value)
    CHECK(n->seq.link_thr == 0.0 || m.images <= 256) << "detect_merge_end: num_frames " << m.images << " is outside [1, 256] while Seq-NMS is on (set_seq_nms link_thr "
                                   << n->seq.link_thr << "): the merge was begun with " << m.images << " lists per slot";
    CHECK(seg_dets != nullptr) << "detect_merge_end: null seg_dets";
    CHECK_GE(m.passes, 1) << "detect_merge_end: no forward has been added since mscnn_net_detect_merge_begin";
    const int S = m.images * m.slots;
    hipStream_t st = (hipStream_t)Caffe::stream();
    const size_t total = mscnn_multi_pack_layout_of(S, S * m.cand_cap).total;
    const bool wbf = n->wbf.thr != 0.0;      // weighted boxes fusion (mscnn_net_set_wbf) in place of the hard merge: the same pack, and
    n->members_valid = false;                // behind it in the same pinned block the member counts, which come over with it
    const bool seq = n->seq.link_thr != 0.0;      // Seq-NMS (mscnn_net_set_seq_nms): the lists are the frames of one clip; the same pack,
                                                  // and the sequence ids where WBF has its member counts (the two are never on together)
    const size_t members_at = (total + 15) / 16 * 16;
    // the tracker (mscnn_net_set_tracker; never on together with WBF): the lists are consecutive frames of the stream; its ids go
    // behind the pack too, behind Seq-NMS's sequence ids when that is on
    const bool track = n->track_on;
    if (track) track_slots_checked(n, "detect_merge_end", m.images, m.slots);
    const size_t per_row = (size_t)S * m.cand_cap * sizeof(int);
    const size_t tracks_at = seq ? (members_at + per_row + 15) / 16 * 16 : members_at;
    ensure_det_host(n, track ? tracks_at + per_row : (wbf || seq) ? members_at + per_row : total);
    *static_cast<volatile int*>(n->det_host) = -1;      // the header's first word: the kernels must have written it
    const bool soft = n->soft.method != 0;      // Soft-NMS (mscnn_net_set_soft_nms) in place of the hard merge: the same pack
    const bool matrix = n->matrix.method != 0;      // Matrix NMS (mscnn_net_set_matrix_nms), likewise; never on together with soft
    const size_t wb = seq ? mscnn_detections_merge_seq_workspace_bytes(m.images, m.slots, m.cand_cap, n->seq.top_k)
                      : wbf ? mscnn_detections_merge_wbf_workspace_bytes(S, m.cand_cap)
                      : matrix ? mscnn_detections_merge_matrix_workspace_bytes(S, m.cand_cap)
                      : soft ? mscnn_detections_merge_soft_workspace_bytes(S, m.cand_cap) : mscnn_detections_merge_workspace_bytes(S, m.cand_cap);
    void* ws = n->det_ws.Reserve(wb);
    // (the merge kernels only ever WRITE the pack: they write it straight into host-coherent pinned memory, as the blocking detect
    // calls do; the vote reads back the table and each kept row's own box from there, in stream order, and nothing else)
    if (seq) {
      MSCNN_CHECK(mscnn_detections_merge_seq_fwd(m.overlap.data(), &n->seq, m.images, m.slots, m.cand.get(), m.cand_cap, n->det_host_dev,
                                                 reinterpret_cast<int*>(static_cast<char*>(n->det_host_dev) + members_at), ws, wb, st));
    } else if (wbf) {
      std::vector<int> expected(S);
      for (int s = 0; s < S; ++s) expected[s] = n->wbf_expected ? n->wbf_expected : std::max(1, m.views[s / m.slots]);
      MSCNN_CHECK(mscnn_detections_merge_wbf_fwd(&n->wbf, expected.data(), S, m.cand.get(), m.cand_cap, n->det_host_dev,
                                                 reinterpret_cast<int*>(static_cast<char*>(n->det_host_dev) + members_at), ws, wb, st));
    } else if (matrix) MSCNN_CHECK(mscnn_detections_merge_matrix_fwd(&n->matrix, S, m.cand.get(), m.cand_cap, n->det_host_dev, ws, wb, st));
    else if (soft) MSCNN_CHECK(mscnn_detections_merge_soft_fwd(m.overlap.data(), &n->soft, S, m.cand.get(), m.cand_cap, n->det_host_dev, ws, wb, st));
    else MSCNN_CHECK(mscnn_detections_merge_fwd(m.overlap.data(), nms_arg(n, false), S, m.cand.get(), m.cand_cap, n->det_host_dev, ws, wb, st));
    if (n->vote_thr != 0.0) {      // box voting (mscnn_net_set_box_voting): the kept rows of that pack, refined in place from the lists
      const mscnn_vote_params vote = {n->vote_thr};
      MSCNN_CHECK(mscnn_detections_merge_vote_fwd(&vote, S, m.cand.get(), m.cand_cap, n->det_host_dev, st));
    }
    if (track)
      track_enqueue(n, "detect_merge_end", m.images, m.slots, n->det_host_dev, S * m.cand_cap,
                    reinterpret_cast<int*>(static_cast<char*>(n->det_host_dev) + tracks_at));
    HIP_CHECK(hipStreamSynchronize(st));
    // A stream-K hand-off that timed out in one of the forwards of this merge can not be answered by a re-run here: the input blob
    // holds the last forward only.  As mscnn_net_detect_end: whole tiles from now on, and the caller submits the forwards again.
    const bool seen_now = n->net->HandoffEventSeen();
    CHECK(!seen_now && n->net->handoff_errors() == m.handoff_errors)
        << "a stream-K hand-off timed out in a forward of this merge (mscnn_net_handoff_state): whole-tile scheduling from now on; the "
           "forwards added since mscnn_net_detect_merge_begin must be run and added again";
    unpack_merge(n->det_host, S, m.cand_cap, dets_host, pass_host, row_host, cap, seg_dets, seg_candidates);
    if (wbf) {      // the counts of the detections just returned, in their order (mscnn_net_detect_merge_members)
      const int* mh = reinterpret_cast<const int*>(static_cast<const char*>(n->det_host) + members_at);
      n->wbf_members.clear();
      for (int s = 0; s < S; ++s) n->wbf_members.insert(n->wbf_members.end(), mh + (size_t)s * m.cand_cap, mh + (size_t)s * m.cand_cap + seg_dets[s]);
      n->wbf_seg_dets.assign(seg_dets, seg_dets + S);
      n->members_valid = true;
    }
    if (seq) {      // the sequence ids of the detections just returned, in their order (mscnn_net_detect_merge_sequences)
      const int* qh = reinterpret_cast<const int*>(static_cast<const char*>(n->det_host) + members_at);
      n->seq_ids.clear();
      for (int s = 0; s < S; ++s) n->seq_ids.insert(n->seq_ids.end(), qh + (size_t)s * m.cand_cap, qh + (size_t)s * m.cand_cap + seg_dets[s]);
      n->seq_seg_dets.assign(seg_dets, seg_dets + S);
      n->sequences_valid = true;
    }
    if (track) {      // the call has succeeded: commit the table, keep the track ids of the detections just returned (mscnn_net_detect_tracks)
      track_commit(n, m.slots);
      const int* th = reinterpret_cast<const int*>(static_cast<const char*>(n->det_host) + tracks_at);
      n->track_ids.clear();
      for (int s = 0; s < S; ++s) n->track_ids.insert(n->track_ids.end(), th + (size_t)s * m.cand_cap, th + (size_t)s * m.cand_cap + seg_dets[s]);
      n->track_seg_dets.assign(seg_dets, seg_dets + S);
      n->tracks_valid = true;
    }
    render_keep(n, m.images, m.slots, S * m.cand_cap, track, tracks_at);
  });
}

// The render stage (mscnn_hip.h: mscnn_render_detections_u8) on the pack the last blocking multi call left in det_host.  The pack and
// the ids go to the stage's own device buffer in one copy (the kernel's workgroups each walk all its rows: not over the bus), host
// frames are staged through the stage's own buffers -- img_in may already hold the next forward's frames.
int mscnn_net_render(mscnn_net* n, const unsigned char* const* frames_rgb, int on_device, const int* org_h, const int* org_w, int count,
                     const mscnn_render_params* p, unsigned char* const* out_rgb, int out_on_device) {
  return guarded([&] {
    CHECK(n && frames_rgb && org_h && org_w && p && out_rgb) << "render: null pointer";
    mscnn_net::Render& r = n->render;
    CHECK(r.valid) << "render: no pack to render: the last call that used the net's pack block was not a successful mscnn_net_detect_multi, "
                      "mscnn_net_detect_cascade_multi or mscnn_net_detect_merge_end";
    CHECK_EQ(count, r.frames) << "render: " << count << " frames, that call had " << r.frames << " images (lists)";
    CHECK(r.ids || (p->label < 2 && p->color_by == 0))
        << "render: label " << p->label << ", color_by " << p->color_by << " need track ids, and that call ran no tracker (mscnn_net_set_tracker)";
    for (int b = 0; b < count; ++b)
      CHECK(frames_rgb[b] && out_rgb[b] && org_h[b] > 0 && org_w[b] > 0)
          << "render: frame " << b << " is " << org_h[b] << " x " << org_w[b] << (frames_rgb[b] && out_rgb[b] ? "" : " at a null pointer");
    hipStream_t st = (hipStream_t)Caffe::stream();
    char* pack = static_cast<char*>(r.pack.Reserve(r.bytes));
    HIP_CHECK(hipMemcpyAsync(pack, n->det_host, r.bytes, hipMemcpyHostToDevice, st));
    std::vector<size_t> off(count + 1, 0);
    for (int b = 0; b < count; ++b) off[b + 1] = off[b] + (((size_t)org_h[b] * org_w[b] * 3 + 255) & ~(size_t)255);
    std::vector<const unsigned char*> src(frames_rgb, frames_rgb + count);
    std::vector<unsigned char*> dst(out_rgb, out_rgb + count);
    if (!on_device) {
      unsigned char* d = static_cast<unsigned char*>(r.in.Reserve(off[count]));
      for (int b = 0; b < count; ++b) {
        HIP_CHECK(hipMemcpyAsync(d + off[b], frames_rgb[b], (size_t)org_h[b] * org_w[b] * 3, hipMemcpyHostToDevice, st));
        src[b] = d + off[b];
      }
    }
    if (!out_on_device) {
      unsigned char* d = static_cast<unsigned char*>(r.out.Reserve(off[count]));
      for (int b = 0; b < count; ++b) dst[b] = d + off[b];
    }
    MSCNN_CHECK(mscnn_render_detections_u8(p, src.data(), dst.data(), org_h, org_w, count, r.slots, pack, r.cap,
                                           r.ids ? reinterpret_cast<const int*>(pack + r.ids_at) : nullptr, st));
    if (!out_on_device) {      // every frame's copy, then the one synchronisation
      for (int b = 0; b < count; ++b)
        HIP_CHECK(hipMemcpyAsync(out_rgb[b], dst[b], (size_t)org_h[b] * org_w[b] * 3, hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
    }
  });
}

// What mscnn_net_crops and mscnn_net_crop_window refuse about the params alone ("" = nothing); of slot only the lower bound can be
// told without a pack.
static std::string crops_params_error(const mscnn_crops_params& p) {
  std::ostringstream e;
  if (p.thr != p.thr) e << "thr is NaN";
  else if (!(p.context >= 1.0 && p.context <= 16.0)) e << "context " << p.context << " is outside [1, 16]";
  else if (p.fit != 0 && p.fit != 1) e << "fit " << p.fit << " is neither 0 nor 1";
  else if (p.border != 0 && p.border != 1) e << "border " << p.border << " is neither 0 (clip) nor 1 (shift)";
  else if (p.min_size < 1) e << "min_size " << p.min_size << " is below 1";
  else if (p.out_h < 1 || p.out_h > 1024) e << "out_h " << p.out_h << " is outside [1, 1024]";
  else if (p.out_w < 1 || p.out_w > 1024) e << "out_w " << p.out_w << " is outside [1, 1024]";
  else if (p.max_crops < 1) e << "max_crops " << p.max_crops << " is below 1";
  else if (p.slot < -1) e << "slot " << p.slot << " is below -1";
  else if (p.tracked_only != 0 && p.tracked_only != 1) e << "tracked_only " << p.tracked_only << " is neither 0 nor 1";
  else
    for (int c = 0; c < 3; ++c)
      if (!std::isfinite(p.mean_bgr[c])) { e << "mean_bgr[" << c << "] " << p.mean_bgr[c] << " is not finite"; break; }
  return e.str();
}

// Steps 1 - 7 of include/mscnn_net.h's comment on mscnn_net_crops, for checked params and a checked frame size.
static int crop_window_of(const mscnn_crops_params& p, const double* row, int org_h, int org_w, int* win) {
#pragma clang fp contract(off)      // one rounding per operation: (x0 + ww) must not become a fused multiply-add of w * context
  const double kMax = 1073741824.0;      // 2^30
  const double x = row[0], y = row[1], w = row[2], h = row[3], s = row[4];
  if (!(s >= p.thr)) return 0;
  if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(w) || !std::isfinite(h) || !std::isfinite(s)) return 0;
  if (!(w > 0.0) || !(h > 0.0)) return 0;
  if (std::fabs(x) > kMax || std::fabs(y) > kMax || w > kMax || h > kMax) return 0;
  double ww = w * p.context;
  double hh = h * p.context;
  if (p.fit == 1) {
    const double a = (double)p.out_w / (double)p.out_h;
    const double t = hh * a;
    if (ww < t) ww = t;
    else hh = ww / a;
  }
  const double hw = w / 2, hw2 = ww / 2;
  const double cx = x + hw;
  const double x0 = cx - hw2;
  const double hv = h / 2, hv2 = hh / 2;
  const double cy = y + hv;
  const double y0 = cy - hv2;
  const double xl = x0 + .5, yt = y0 + .5;
  const double x1 = x0 + ww, y1 = y0 + hh;
  const double xr = x1 + .5, yb = y1 + .5;
  long long L = (long long)std::floor(xl), T = (long long)std::floor(yt);      // (|values| < 2^46: exact)
  const long long R = (long long)std::floor(xr) - 1, B = (long long)std::floor(yb) - 1;
  long long Wd = R - L + 1, Ht = B - T + 1;
  if (Wd < 1 || Ht < 1) return 0;
  if (p.border == 1) {
    if (Wd >= org_w) { L = 0; Wd = org_w; }
    else if (L < 0) L = 0;
    else if (L + Wd > org_w) L = org_w - Wd;
    if (Ht >= org_h) { T = 0; Ht = org_h; }
    else if (T < 0) T = 0;
    else if (T + Ht > org_h) T = org_h - Ht;
  } else {
    const long long L1 = std::max(L, 0LL), R1 = std::min(R, (long long)org_w - 1);
    const long long T1 = std::max(T, 0LL), B1 = std::min(B, (long long)org_h - 1);
    if (L1 > R1 || T1 > B1) return 0;
    L = L1; T = T1; Wd = R1 - L1 + 1; Ht = B1 - T1 + 1;
  }
  if (Wd < p.min_size || Ht < p.min_size) return 0;
  win[0] = (int)L; win[1] = (int)T; win[2] = (int)Wd; win[3] = (int)Ht;
  return 1;
}

int mscnn_net_crop_window(const mscnn_crops_params* p, const double row[5], int org_h, int org_w, int win[4]) {
  std::ostringstream e;
  if (!p || !row || !win) e << "null pointer";
  else if (org_h <= 0 || org_w <= 0 || org_h > (1 << 30) || org_w > (1 << 30)) e << "the frame is " << org_h << " x " << org_w;
  else e << crops_params_error(*p);
  if (!e.str().empty()) {
    g_err = "crop_window: " + e.str();
    return -1;
  }
  return crop_window_of(*p, row, org_h, org_w, win);
}

// Every detection of the pack the last blocking multi call left in det_host as a patch: the host walks the pack (it lies in pinned
// host memory) and computes the windows, the views op cuts and resizes them in one call.  Host frames are staged through the stage's
// own buffer -- img_in may already hold the next forward's frames -- and only those that have a crop.
int mscnn_net_crops(mscnn_net* n, const unsigned char* const* frames_rgb, int on_device, const int* org_h, const int* org_w, int count,
                    const mscnn_crops_params* p, float* out, int out_on_device, mscnn_crop_info* info_host, int* num_crops,
                    int* num_dropped) {
  return guarded([&] {
    CHECK(n && frames_rgb && org_h && org_w && p && out && info_host && num_crops && num_dropped) << "crops: null pointer";
    CHECK_GE(n->device, 0) << "crops: the net was built with device " << n->device << " (graph only)";
    const mscnn_net::Render& r = n->render;
    CHECK(r.valid) << "crops: no pack to cut from: the last call that used the net's pack block was not a successful mscnn_net_detect_multi, "
                      "mscnn_net_detect_cascade_multi or mscnn_net_detect_merge_end";
    CHECK_EQ(count, r.frames) << "crops: " << count << " frames, that call had " << r.frames << " images (lists)";
    for (int b = 0; b < count; ++b)
      CHECK(frames_rgb[b] && org_h[b] > 0 && org_w[b] > 0 && org_h[b] <= (1 << 30) && org_w[b] <= (1 << 30))
          << "crops: frame " << b << " is " << org_h[b] << " x " << org_w[b] << (frames_rgb[b] ? "" : " at a null pointer");
    const std::string bad = crops_params_error(*p);
    CHECK(bad.empty()) << "crops: " << bad;
    CHECK(p->slot < r.slots) << "crops: slot " << p->slot << " is outside [-1, " << r.slots << ")";
    CHECK(r.ids || p->tracked_only == 0) << "crops: tracked_only " << p->tracked_only
                                         << " needs track ids, and that call ran no tracker (mscnn_net_set_tracker)";
    // the windows, in the order (frame, slot, row)
    const int K = r.slots;
    const char* pack = static_cast<const char*>(n->det_host);
    const int* hdr = reinterpret_cast<const int*>(pack);
    const double* rows = reinterpret_cast<const double*>(pack + mscnn_multi_pack_layout_of(r.frames * K, r.cap).dets);
    const int* ids = r.ids ? reinterpret_cast<const int*>(pack + r.ids_at) : nullptr;
    std::vector<mscnn_preprocess_view> views;
    std::vector<int> place(count, -1);      // frame -> its place among the frames that have a crop
    int dropped = 0;
    for (int b = 0; b < count; ++b) {
      const int* e0 = hdr + MSCNN_MULTI_PACK_WORDS * (size_t)(1 + b * K);
      const bool shared = K >= 2 && e0[2] == e0[MSCNN_MULTI_PACK_WORDS + 2];
      for (int k = p->slot < 0 ? 0 : p->slot; k < (p->slot < 0 ? K : p->slot + 1); ++k) {
        const int* e = e0 + MSCNN_MULTI_PACK_WORDS * (size_t)k;
        const long long cnt = e[0], off = shared ? (long long)K * e[2] + (long long)k * e[1] : (long long)e[2];
        if (cnt < 0 || off < 0 || off + cnt > r.cap) continue;
        for (long long j = 0; j < cnt; ++j) {
          const int id = ids ? ids[off + j] : 0;
          if (p->tracked_only && !(id > 0)) continue;
          int win[4];
          const int rc = mscnn_net_crop_window(p, rows + 5 * (off + j), org_h[b], org_w[b], win);
          CHECK_GE(rc, 0) << g_err;
          if (rc == 0) continue;
          if ((int)views.size() >= p->max_crops) { ++dropped; continue; }
          if (place[b] < 0) place[b] = 0;
          info_host[views.size()] = mscnn_crop_info{b, k, (int)j, id, win[0], win[1], win[2], win[3]};
          views.push_back(mscnn_preprocess_view{b, win[0], win[1], win[2], win[3], 0});
        }
      }
    }
    *num_crops = (int)views.size();
    *num_dropped = dropped;
    if (views.empty()) return;
    // the frames that have a crop, each once
    std::vector<const unsigned char*> src;
    std::vector<int> hs, ws;
    std::vector<size_t> off(1, 0);
    for (int b = 0; b < count; ++b) {
      if (place[b] < 0) continue;
      place[b] = (int)src.size();
      src.push_back(frames_rgb[b]); hs.push_back(org_h[b]); ws.push_back(org_w[b]);
      off.push_back(off.back() + (((size_t)org_h[b] * org_w[b] * 3 + 255) & ~(size_t)255));
    }
    for (mscnn_preprocess_view& v : views) v.frame = place[v.frame];
    hipStream_t st = (hipStream_t)Caffe::stream();
    const int F = (int)src.size(), V = (int)views.size();
    if (!on_device) {
      unsigned char* d = static_cast<unsigned char*>(n->crops.in.Reserve(off[F]));
      for (int f = 0; f < F; ++f) {
        HIP_CHECK(hipMemcpyAsync(d + off[f], src[f], (size_t)hs[f] * ws[f] * 3, hipMemcpyHostToDevice, st));
        src[f] = d + off[f];
      }
    }
    const size_t wb = mscnn_preprocess_views_workspace_bytes(views.data(), V, p->out_h, p->out_w);
    void* wsp = n->crops.ws.Reserve(wb);
    const size_t bytes = (size_t)V * 3 * p->out_h * p->out_w * sizeof(float);
    float* dst = out_on_device ? out : static_cast<float*>(n->crops.out.Reserve(bytes));
    MSCNN_CHECK(mscnn_preprocess_views_u8_f32(src.data(), hs.data(), ws.data(), F, views.data(), V, dst, p->out_h, p->out_w, p->mean_bgr,
                                              wsp, wb, st));
    if (!out_on_device) {      // the patches in one copy, then the one synchronisation
      HIP_CHECK(hipMemcpyAsync(out, dst, bytes, hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
    }
  });
}

int mscnn_net_detect_merge_sequences(mscnn_net* n, int* seq_host, int cap, const int* seg_dets) {
  return guarded([&] {
    CHECK(n != nullptr);
    CHECK(n->sequences_valid) << "detect_merge_sequences: the last mscnn_net_detect_merge_end did not run Seq-NMS (mscnn_net_set_seq_nms was "
                                 "off, the call failed, or there was none)";
    CHECK(seg_dets != nullptr) << "detect_merge_sequences: null seg_dets";
    const size_t S = n->seq_seg_dets.size();
    for (size_t s = 0; s < S; ++s)
      CHECK_EQ(seg_dets[s], n->seq_seg_dets[s]) << "detect_merge_sequences: segment " << s << ": seg_dets " << seg_dets[s]
                                                << ", that _end returned " << n->seq_seg_dets[s];
    const size_t D = n->seq_ids.size();
    CHECK_LE(D, (size_t)(cap < 0 ? 0 : cap)) << "detect_merge_sequences: the buffer holds " << cap << " ids, that _end returned " << D << " detections";
    CHECK(D == 0 || seq_host) << "detect_merge_sequences: null sequence buffer";
    if (D) std::memcpy(seq_host, n->seq_ids.data(), D * sizeof(int));
  });
}

int mscnn_net_detect_merge_members(mscnn_net* n, int* members_host, int cap, const int* seg_dets) {
  return guarded([&] {
    CHECK(n != nullptr);
    CHECK(n->members_valid) << "detect_merge_members: the last mscnn_net_detect_merge_end did not run weighted boxes fusion (mscnn_net_set_wbf "
                               "was off, the call failed, or there was none)";
    CHECK(seg_dets != nullptr) << "detect_merge_members: null seg_dets";
    const size_t S = n->wbf_seg_dets.size();
    for (size_t s = 0; s < S; ++s)
      CHECK_EQ(seg_dets[s], n->wbf_seg_dets[s]) << "detect_merge_members: segment " << s << ": seg_dets " << seg_dets[s] << ", that _end returned "
                                                << n->wbf_seg_dets[s];
    const size_t D = n->wbf_members.size();
    CHECK_LE(D, (size_t)(cap < 0 ? 0 : cap)) << "detect_merge_members: the buffer holds " << cap << " counts, that _end returned " << D << " detections";
    CHECK(D == 0 || members_host) << "detect_merge_members: null members buffer";
    if (D) std::memcpy(members_host, n->wbf_members.data(), D * sizeof(int));
  });
}

}  // extern "C"
