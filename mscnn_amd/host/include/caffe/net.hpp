// Net<Dtype>: graph build + sequential executor (mirror of include/caffe/net.hpp / src/caffe/net.cpp for
// the TEST-phase forward path): legacy `input:` upgrade, automatic Split insertion with the reference's
// blob/layer naming, in-place tops, by-name lookup, outputs = un-consumed blobs in alphabetical order.
#ifndef MSCNN_CAFFE_NET_HPP_
#define MSCNN_CAFFE_NET_HPP_

#include <map>
#include <utility>
#include <set>
#include <string>
#include <vector>

#include "caffe/blob.hpp"
#include "caffe/common.hpp"
#include "caffe/layer.hpp"
#include "caffe/proto/caffe_param.hpp"

namespace caffe {

template <typename Dtype> class ConvolutionLayer;
template <typename Dtype> class InnerProductLayer;
template <typename Dtype> class ROIPoolingLayer;

// Applied by Net::Init before layers are created (mirrors UpgradeNetInput + InsertSplits).
void UpgradeNetInput(const NetParameter& in, vector<LayerParameter>* layers);
void InsertSplits(const vector<LayerParameter>& in, vector<LayerParameter>* out);

template <typename Dtype>
class Net {
 public:
  // fusion: Net-level operator fusion (ReLU / MAX 2x2 pooling into the producing convolution, ROIPooling -> Concat).  On by
  // default; the process-wide default can be turned off with MSCNN_NO_FUSE=1 (results are bit-identical either way).
  explicit Net(const NetParameter& param, Phase phase = TEST);
  explicit Net(const string& param_file, Phase phase);
  Net(const NetParameter& param, Phase phase, bool fusion);
  virtual ~Net();

  const vector<Blob<Dtype>*>& Forward(Dtype* loss = NULL);
  const vector<Blob<Dtype>*>& ForwardPrefilled(Dtype* loss = NULL) { return Forward(loss); }
  Dtype ForwardFromTo(int start, int end);
  void Reshape();

  // Loads weights by layer name from a binary NetParameter (.caffemodel), net.cpp:750-803; a name ending in ".h5" is read as
  // an HDF5 snapshot like the reference does (net.cpp:788-795, 806-848).
  void CopyTrainedLayersFrom(const string& trained_filename);
  void CopyTrainedLayersFromHDF5(const string& trained_filename);
  // Must be called after parameter blobs were written through mutable_cpu_data()/mutable_gpu_data().
  void MarkWeightsChanged();

  inline const string& name() const { return name_; }
  inline const vector<string>& layer_names() const { return layer_names_; }
  inline const vector<string>& blob_names() const { return blob_names_; }
  inline const vector<shared_ptr<Blob<Dtype> > >& blobs() const { return blobs_; }
  inline const vector<shared_ptr<Layer<Dtype> > >& layers() const { return layers_; }
  inline const vector<vector<Blob<Dtype>*> >& bottom_vecs() const { return bottom_vecs_; }
  inline const vector<vector<Blob<Dtype>*> >& top_vecs() const { return top_vecs_; }
  inline int num_inputs() const { return (int)net_input_blobs_.size(); }
  inline int num_outputs() const { return (int)net_output_blobs_.size(); }
  inline const vector<Blob<Dtype>*>& input_blobs() const { return net_input_blobs_; }
  inline const vector<int>& input_blob_indices() const { return net_input_blob_indices_; }
  // number of ForwardFromTo calls so far (readers that cache something derived from the blobs key it on this)
  long forward_count() const { return forward_count_; }
  inline const vector<Blob<Dtype>*>& output_blobs() const { return net_output_blobs_; }
  inline const vector<int>& output_blob_indices() const { return net_output_blob_indices_; }
  bool has_blob(const string& blob_name) const;
  const shared_ptr<Blob<Dtype> > blob_by_name(const string& blob_name) const;
  bool has_layer(const string& layer_name) const;
  const shared_ptr<Layer<Dtype> > layer_by_name(const string& layer_name) const;

  // --- extensions of this build ---
  // Conv/InnerProduct + in-place ReLU fusion is decided at construction: on by default, MSCNN_NO_FUSE=1 disables it.
  const vector<bool>& layer_fused_away() const { return fused_away_; }
  // Per-layer HIP-event timing of the last Forward when enabled (the `caffe time` loop, tools/caffe.cpp:380-400).
  void set_layer_timing(bool on) { timing_ = on; }
  const vector<float>& layer_ms() const { return layer_ms_; }
  // Tops whose producer was redirected into a fused Concat's top (roi_pool_org / roi_pool_ctx) are materialised lazily:
  // blob_by_name() copies the channel window back into the blob's own storage when the producer has run since the last
  // copy.  Code that reaches into blobs() directly must call this first.
  void MaterializeBlob(int blob_id) const;
  // Deferred ROI pooling (ROIPoolingLayer::set_deferred): the pair's blob is written now if it is still pending and `blob_name` is
  // (or shares its data, through Split layers, with) a blob the pooling reads; likewise the unwritten blobs of convolution chains and
  // ROIAlign heads that hang on it.  Call before writing -- from outside the Net -- into a blob (the C ABI's blob setters do).
  void MaterializePendingReadersOf(const string& blob_name) const;
  // Chains of same-resolution F(4x4,3x3) convolutions (ConvolutionLayer::ChainTo: conv2_1 -> conv2_2, conv3_1 -> 3_2 -> 3_3,
  // conv4_1 -> 4_2 -> 4_3): the blob between two members is not written while both run in one ForwardFromTo call; blob_by_name()
  // / MaterializeBlob() re-run the producer unchained when somebody asks for it (bit-identical).  On by default with `fusion`;
  // MSCNN_NO_CHAIN=1 or SetChainFusion(false) turn it off (every blob is then written by every Forward).
  void SetChainFusion(bool on) { chain_fusion_ = on; }
  // Every blob the last Forward left unwritten is written now (the weights are about to change: what the blobs hold must stay what
  // the layers computed with the OLD weights, as in the reference).  Called by the weight loaders and the C ABI's parameter setter.
  void MaterializeStale() const;
  bool chain_fusion() const { return chain_fusion_; }
  // (producer layer, consumer layer or -1 for a top read by its fused pooling only) of every registered pair
  vector<std::pair<int, int> > chain_pairs() const {
    vector<std::pair<int, int> > out;
    for (size_t k = 0; k < chain_pairs_.size(); ++k) out.push_back(std::make_pair(chain_pairs_[k].producer, chain_pairs_[k].consumer));
    return out;
  }
  // The ROIAlign head in one pass.  A head is registered at construction (with or without `fusion`): two ROIAlign layers that read
  // the same feature blob and the same ROI blob (through Split layers) with equal pooled_h / pooled_w / spatial_scale, each top read by
  // exactly one Pooling layer that is AVE 2x2 / stride 1 / pad 0, those two tops read only by one Concat on axis 1 (roi_grid_org /
  // roi_pool_org / roi_grid_ctx / roi_pool_ctx / roi_pool of the WiderFace cascade, once per stage).  OFF by default: nothing changes
  // for a net that never calls this.  ON: in a ForwardFromTo whose range holds all five layers the first ROIAlign layer writes the
  // Concat's top with one launch (ROIAlignLayer::PairWith) and the other four launch nothing; the two grid blobs and the two pooled
  // blobs are then written on demand -- blob_by_name() / MaterializeBlob() / MaterializeStale() run the four skipped layers on the same
  // bottoms, the very kernels the switch-off path runs --, and before a later call that does not run the whole head could change what
  // they read.  A range that holds only part of a head runs its layers stand-alone.
  void SetRoiAlignOnePass(bool on) { roialign_one_pass_ = on; }
  bool roialign_one_pass() const { return roialign_one_pass_; }
  // the first ROIAlign layer of every registered head
  vector<int> roialign_pairs() const {
    vector<int> out;
    for (size_t k = 0; k < align_heads_.size(); ++k) out.push_back(align_heads_[k].layer[0]);
    return out;
  }
  // Numerical calibration on representative data: call after a Forward.  Every Convolution layer that runs a Winograd
  // form is re-computed with the direct k-ordered kernel on the same bottom (ConvolutionLayer::ErrorAgainstDirect); where
  // max |dy| / max(1, |y|, rms(y)) exceeds `tol` the layer is switched to the direct kernel for good (FallBackIfStrayed).  Returns the
  // layers switched; errors (per layer index, 0 for layers not checked) are left in calibration_err().
  vector<int> CalibrateNumerics(double tol);
  const vector<double>& calibration_err() const { return calib_err_; }
  // Safe by default (no call needed): every Convolution layer checks its Winograd result against the direct kernel by itself on the
  // first Forward after construction / CopyTrainedLayersFrom / MarkWeightsChanged and falls back before that Forward returns
  // (ConvolutionLayer::set_selfcheck); the Net only keeps the books -- calibration_err(), auto_calibrate_checks / _switched -- and
  // offers the opt-OUT: SetAutoCalibrate(0).  tol > 0 re-arms the check on every layer with that tolerance.
  void SetAutoCalibrate(double tol);
  int auto_calibrate_checks() const { return auto_checks_; }
  const vector<int>& auto_calibrate_switched() const { return auto_switched_; }
  // The same comparison while a stream of frames runs (the numerics watch): every `period`-th whole Forward looks at ONE Winograd
  // layer (round robin) -- its bottom and top are written as blobs in that frame although it stays in its convolution chain, and the
  // layer's next band (a few rows / images: ~30 us of direct-kernel work; each layer goes round its own bands, one per visit) is
  // recomputed with the direct kernel BEHIND the frame on the same stream (ConvolutionLayer::BeginCheck(kBand)), without a host
  // synchronisation.  The verdict is collected by a later Forward (or by the state accessors below); a layer that strayed by more
  // than tol runs the direct kernel for good from the frame after.  A watch frame costs up to two extra blob writes plus that band
  // (2 - 8 % of a 7s-576 frame); no frame ever waits for a check.  ON by default (every
  // kDefaultWatchPeriod-th frame, tolerance 5e-5: ~0.1 % of a stream); period 0 turns it off.
  static constexpr int kDefaultWatchPeriod = 25;
  void SetNumericsWatch(int period, double tol);
  // (both wait for a verdict that is still out, so that what they return is final for the frames forwarded so far)
  int numerics_watch_checks() { WatchCollect(true); return watch_checks_; }
  const vector<int>& numerics_watch_switched() { WatchCollect(true); return watch_switched_; }
  void WatchCollect(bool wait);
  // Health of the plane-GEMM kernel's stream-K hand-off (include/mscnn_hip.h: mscnn_wgemm_handoff_event).  A launch whose finisher
  // gave up on a contributor leaves a NaN tile behind and its tag in a pinned status word; the Net looks at that word wherever the
  // stream has just been synchronised anyway -- behind BoxOutput's row-count read inside ForwardFromTo (covers the trunk and the
  // heads, whose NaN scores BoxOutput would otherwise silently drop) and, through HandoffRecover(), behind the final stage's / a blob
  // read's synchronisation (covers roi_c1 and fc6).  The answer is always the same: whole-tile scheduling for the rest of the
  // process (mscnn_wgemm_force_whole_tiles) and the affected range once more.  handoff_errors() = how often that happened.
  //   HandoffRecover(): call right after synchronising Caffe::stream() on outputs of the last ForwardFromTo.  false = nothing was
  //   reported; true = the range has been run again (asynchronously, like any Forward): read the outputs again.
  bool HandoffRecover();
  // The detection sub-net on caller-supplied ROIs (include/mscnn_net.h: mscnn_net_forward_rois).  L = the BoxOutput layer that feeds
  // the ROI layers, K = the last layer in front of L that a layer behind L depends on other than through L's tops (relu4_3 and the
  // Split behind it in the KITTI / Caltech deploys).  Order of work: the ingest into L's tops (BoxOutputLayer::IngestBegin; blobs that
  // an earlier forward left pending on the ROI blob are written first), ForwardFromTo(0, K) when run_trunk, the wait for the ingest's
  // verdict -- a bad row is a CHECK failure naming row and reason, and the sub-net does not run --, ForwardFromTo(L + 1, last).  The layers
  // between K and L never run.  rows / coords / ratios: mscnn_rois_ingest_f32's; image_rois [num_images] may be null.  Everything
  // that can be refused is refused before anything is enqueued.  While such a frame is the last one run, HandoffRecover() runs the
  // same two ranges again around the ingested rows (they are still in L's tops) instead of one range that would hold L.
  void ForwardRois(const void* rows, bool on_device, int coords, int R, const double* ratio_h, const double* ratio_w, int num_images,
                   bool run_trunk, int* image_rois);
  // L and K of ForwardRois (-1, -1 for a net that has no ROI layer fed by a BoxOutput layer)
  void RoisLayers(int* L, int* K) const;
  // For callers that pipeline frames and therefore can NOT have a range run again (mscnn_net_detect_end): true when a hand-off event
  // was raised since the last look -- whole tiles are forced and the event is counted as in HandoffRecover, nothing is re-run.
  // (the stream is synchronised only up to the frame being collected: what was enqueued behind it stays "unchecked in flight")
  bool HandoffEventSeen() { return HandoffEventPending(); }
  int handoff_errors() const { return handoff_errors_; }

 protected:
  void Init(const NetParameter& param);
  // The graph index: built once by Init behind the wiring loop (BuildGraphIndex), never changed afterwards.  Every pass below that asks
  // "who writes / reads this blob" looks it up here; the predicates on top of it (before which layer, with or without fused-away
  // layers, a net output as a reader) differ from site to site and stay at the sites.
  void BuildGraphIndex();
  vector<vector<int> > blob_writers_;      // blob -> the layers that write it, ascending, in-place writers included
  vector<vector<int> > blob_readers_;      // blob -> the layers that read it, ascending, one entry per bottom occurrence
  vector<bool> blob_is_output_;            // blob -> it is a net output
  vector<int> split_source_;               // blob -> through Split layers (their tops share the bottom's data) the blob that holds the data
  template <typename L> struct Typed { int index; L* layer; };
  vector<Typed<ConvolutionLayer<Dtype> > > conv_layers_;
  vector<Typed<InnerProductLayer<Dtype> > > ip_layers_;
  vector<Typed<ROIPoolingLayer<Dtype> > > roipool_layers_;
  int LastWriter(int blob) const { return blob_writers_[blob].empty() ? -1 : blob_writers_[blob].back(); }
  int LastWriterBefore(int blob, int layer) const;
  // the readers of `blob` that still run (not fused away), `except` left out: their number, the last one in *reader (-1: none)
  int RunningReaders(int blob, int except, int* reader) const;
  int SplitSource(int blob) const { return split_source_[blob]; }
  bool SameData(int blob_a, int blob_b) const { return split_source_[blob_a] == split_source_[blob_b]; }
  // Net-level fusion: four passes in this order (each reads fused_away_ as the earlier ones left it)
  void ApplyFusion();
  void FuseReLUs();
  void FuseMaxPools();
  void FuseRoiPoolConcats();
  void PairRoiPools(int concat_layer);
  void DeferRoiPoolPair(int first, int second, int concat_blob);
  void PrebuildRoiMapsUnderBoxOutput(int pool_layer, int conv_layer);
  void ChainConvolutions();
  // the per-call marks of ForwardFromTo (ROIPooling skip, deferred poolings, max |x| hand-over, ROIAlign heads, convolution chains,
  // the watch layer's keep_top): armed for a range at the head of a call, cleared at its end -- and at its head, for a call that
  // follows one a CHECK failure cut short
  void ArmCallMarks(int start, int end, int watch_layer);
  void ClearCallMarks();
  // max |x| hand-over for split-fp16 convolutions (ConvolutionLayer::set_amax_io): one device slot per layer; a blob's bound
  // follows it through Split / in-place ReLU / Dropout / MAX pooling / ROIPooling / Concat of blobs with one common source.
  void WireAmax();
  void* amax_slots_ = nullptr;
  vector<int> amax_src_;          // convolution layer -> the convolution layer whose max |y| bounds its bottom, or -1

  string name_;
  Phase phase_;
  vector<shared_ptr<Layer<Dtype> > > layers_;
  vector<string> layer_names_;
  std::map<string, int> layer_names_index_;
  vector<shared_ptr<Blob<Dtype> > > blobs_;
  vector<string> blob_names_;
  std::map<string, int> blob_names_index_;
  vector<vector<Blob<Dtype>*> > bottom_vecs_;
  vector<vector<int> > bottom_id_vecs_;
  vector<vector<Blob<Dtype>*> > top_vecs_;
  vector<vector<int> > top_id_vecs_;
  vector<int> net_input_blob_indices_, net_output_blob_indices_;
  vector<Blob<Dtype>*> net_input_blobs_, net_output_blobs_;
  vector<bool> fused_away_;
  bool fusion_, timing_;
  vector<float> layer_ms_;
  // fused layer i -> the layers that now produce its top(s) (ReLU / Pooling: one convolution; Concat: the ROIPooling layers)
  vector<vector<int> > fused_producers_;
  // (dirty: the producer ran since the last MaterializeBlob)
  struct Redirect { int target_blob, c_total, c_offset; mutable bool dirty; };
  std::map<int, Redirect> redirect_;               // blob id -> where its data really lives
  struct DeferredPool { int first_layer, conv_layer, blob; };      // a ROIPooling pair whose only reader pools in its own input stage
  vector<DeferredPool> deferred_pools_;
  struct ChainPair { int producer, consumer, blob; };              // convolution -> its only reader, a same-resolution 3x3 convolution (-1: read by its fused pooling only)
  vector<ChainPair> chain_pairs_;
  bool chain_fusion_ = true;
  // layer: ROIAlign, ROIAlign, their Pooling layers, the Concat (the ROIAlign layers in net order); blob: the two grid blobs and the
  // two pooled blobs; stale: the last forward of the head was the one-pass launch and those four blobs have not been written since
  struct AlignHead { int layer[5]; int blob[4]; int first, last; mutable bool stale; bool live; };
  vector<AlignHead> align_heads_;
  vector<int> layer_head_, layer_head_role_;      // layer -> its head in align_heads_ and its place in AlignHead::layer, or -1
  bool roialign_one_pass_ = false;
  void FindRoiAlignHeads();
  void MaterializeAlignHead(const AlignHead& h) const;
  vector<double> calib_err_;
  int NextWatchLayer() const;
  void FallBackIfStrayed(int layer, double err, double tol, const char* where, vector<int>* switched);
  int watch_period_ = kDefaultWatchPeriod, watch_frame_ = 0, watch_next_ = 0, watch_checks_ = 0;
  int watch_pending_ = -1;      // layer whose band check is in flight (-1: none)
  double watch_tol_ = 5e-5;
  int auto_checks_ = 0;
  double auto_tol_ = 5e-5;      // (= ConvolutionLayer::kDefaultSelfcheckTol; 0 once SetAutoCalibrate(0) opted out)
  vector<int> auto_switched_;
  vector<int> watch_switched_;
  bool HandoffEventPending();      // (the stream must have been synchronised) a new tag in the status word: whole tiles forced, counted
  unsigned long long handoff_seen_ = 0;
  int handoff_errors_ = 0;
  int last_start_ = 0, last_end_ = -1;
  int suspect_start_ = -1;      // smallest `start` of the ranges run since the last synchronisation point that saw no hand-off event (-1: none)
  long forward_count_ = 0;
  // the frame in flight is a ForwardRois: its two ranges (rois_trunk_: the first one ran) for HandoffRecover
  bool rois_frame_ = false, rois_trunk_ = false, in_rois_call_ = false;
  void FindRoisLayers();
  int rois_K_ = -1, rois_L_ = -1;      // L and K of ForwardRois: the graph's, found once by Init
  DISABLE_COPY_AND_ASSIGN(Net);
};

}  // namespace caffe
#endif
