#!/usr/bin/env python3
"""The reference's KITTI demo driver (examples/kitti_car/run_mscnn_detection.m, and run_mscnn_detection.m of kitti_ped_cyc /
caltech: same flow, other class lists) on the MI355X path: net from a deploy prototxt + weight file, every image of a directory
resized / BGR / mean-subtracted ON THE DEVICE (:64-69), net.forward timed alone like the reference's tic / toc (:72-73), the
MATLAB post-processing block (:75-120) as ONE call per class (mscnn_net_detect), the result file
detections/<comp_id>_<class>.txt written as dlmwrite does (:150-161), optionally the per-image KITTI label files of
examples/kitti_result/writeDetForEval.m.

  python tools/run_mscnn_detection.py --prototxt mscnn_deploy.prototxt --weights model.caffemodel --images /KITTI/testing/image_2
         [--out detections] [--comp-id kitti_7s_576] [--cls-ids 2] [--names bg,car,van,truck,tram] [--precision f32|f16x3|f16]
         [--labels-dir results/data] [--limit N] [--batch B]
         [--proposals-out proposals] [--proposals-only]      # the proposal half of the result: proposals/<comp_id>.txt (:154, :161-162)
         [--rois-in FILE]                                    # the detection sub-net on these boxes instead of the net's own proposals
         [--nms-type maxg|max] [--ovr-dnm union|min] [--nms-thr T] [--det-thr T]      # pNms.type / pNms.ovrDnm / bbNms's thr, and
                                                             # the det_thr of the WiderFace plain flow (Net.set_nms, once per run)
         [--scales H1xW1,H2xW2,...] [--flip] [--merge-cap N] # several forwards per frame, one NMS (Net.detect_merge_*)
         [--tiles RxC[:overlap_px]] [--views-batch]          # the frame cut into tiles; all views of a frame as ONE batched forward
         [--vote [THR]]                                      # box voting behind the merged NMS (Net.set_box_voting, THR default 0.5)
         [--soft-nms linear|gaussian[:SIGMA]] [--soft-thr T] [--max-dets N]      # Soft-NMS in place of the merged NMS (Net.set_soft_nms)
         [--matrix-nms linear|gaussian[:SIGMA]]              # Matrix NMS in its place instead (Net.set_matrix_nms); --soft-thr / --max-dets serve it
         [--wbf [THR]] [--wbf-skip T] [--wbf-conf avg|max] [--wbf-expected N]      # weighted boxes fusion in its place instead (Net.set_wbf)
         [--seq-nms [avg|max]] [--clip T] [--seq-link THR] [--seq-top-k N] [--tubelets-out DIR]      # Seq-NMS over clips of T frames (Net.set_seq_nms)
         [--track] [--track-high T] [--track-low T] [--track-match THR] [--track-motion none|linear|kalman] [--track-max-age N] [--track-min-hits N]
         [--track-kalman-pos S] [--track-kalman-vel S] [--track-kalman-keep-height 0|1]      # with --track-motion kalman (Net.set_tracker_kalman)
         [--track-assign greedy|optimal]                                                     # with --track (Net.set_tracker_assign)
         [--tracks-out DIR]                                  # track ids across the frames of the run (Net.set_tracker)
         [--track --streams N --batch B]                     # the frames are N multiplexed cameras: a table of tracks per camera
         [--render-out DIR] [--show-thr T] [--render-label none|score|id|both] [--render-color slot|id] [--pixelate N]
                                                             # the scripts' `show` block on the device (Net.render): annotated PNGs
         [--crops-out DIR] [--crop-size HxW] [--crop-thr T] [--crop-context F] [--crop-fit] [--crop-border clip|shift] [--crop-min N]
         [--crop-tracked]                                    # every detection as a fixed-size patch, cut on the device (Net.crops)
  python tools/run_mscnn_detection.py --model kitti_car/mscnn-7s-576 --synthetic 8      # no dataset / weights at hand: the generated
                                                                                        # deploy net, seeded weights, synthetic frames

--batch B > 1 runs B frames per forward: the net's input is reshaped to (B, 3, H, W) (the last group to its own size), the group is
pre-processed in one call (Net.set_images) and its final stage runs for every frame and class in one pass (Net.detect_multi); the
output files are the same, avgtime stays per frame.

--proposals-out DIR also writes what the scripts build as final_proposals (:75-91, :154, :161-162 -- the dlmwrite the reference ships
commented out): DIR/<comp_id>.txt, rows [image_index x y w h score], every image's proposals filtered as the final stage filters them
and rescaled to the original image (Net.proposals_multi: one pass per forward, batch 1 and --batch B).  --proposals-only runs MS-CNN
as a proposal generator: the layers up to BoxOutput (Net.forward_proposals), no detect call, no detection files.

--rois-in FILE runs the other half alone: rows [image_index x y w h score] in original-image pixels, image_index 1-based over the
frames of the run in ascending order -- the format --proposals-out writes -- go through Net.forward_rois instead of Net.forward, per
frame or per --batch group (conv5_x, the proposal heads and BoxOutput never run); everything behind the forward is unchanged.  A frame
without rows gets no detections; a group in which no frame has rows is not forwarded at all.  Not together with --proposals-only.

--scales / --flip run every frame more than once -- at each of the given input sizes (the net's input is reshaped), and with --flip
a second time mirrored on the host ([:, ::-1]) -- and merge the candidates of all those forwards before ONE NMS per class: per frame one
Net.detect_merge_begin, per forward set_image + forward + Net.detect_merge_add (the mirrored one with the view flip_x = 1), then one
Net.detect_merge_end.  The candidate lists hold (forwards per frame) x BoxOutput's max_nms_num rows (--merge-cap N: another number; it
is needed for a deploy without a max_nms_num).  One frame per forward; not with --batch, --rois-in or the proposal outputs.  The
result files have the same layout.  No reference script does this: there is no pin on the reference for it.  Without these flags the
driver runs exactly the calls it ran before they existed.

--tiles RxC[:overlap_px] cuts every frame into R x C equal windows that overlap by that many pixels (mscnn_amd.net.tile_views: the
last row and column are shifted inwards, not shrunk), runs each as a view -- the window is resized to the net's input on the device
straight out of the uploaded frame (Net.set_image_views), no crop on the host --, with --flip each tile's mirror too, and merges all
of them before ONE NMS per class.  --views-batch (with --flip and/or --tiles) runs all views of a frame in ONE forward: the input is
reshaped to N images, one set_image_views (the frame is uploaded once), one forward, one detect_merge_add(..., list_of=), one
detect_merge_end; without it the views run as single forwards.  With --scales the same per input size.  No reference script has
views: there is no pin on the reference for them either.

--vote [THR] (default 0.5) refines every kept box behind the merged NMS: it becomes the score-weighted mean of all candidates of its
class and frame -- from every forward -- whose IoU with it is >= THR (Net.set_box_voting, once per run; the vote runs on the device
between the merge and its read-back).  Alongside --scales / --flip / --tiles it votes over their forwards; without them the frame
runs as a merge of ONE forward, so the vote is there for a single forward too (its candidates are the rows the NMS suppressed).  No
reference script votes: there is no pin on the reference for it.

--soft-nms linear|gaussian[:SIGMA] runs Soft-NMS (Bodla et al., 2017) in place of the merged hard NMS, on the device
(Net.set_soft_nms, once per run): a candidate that overlaps a picked box is not deleted, its score is decayed -- linear: by 1 - IoU
where the IoU is above --nms-overlap; gaussian: by exp(-IoU^2 / SIGMA), SIGMA defaults to 0.5 -- and the detections come out with
their decayed scores; --soft-thr T (default 0.001) ends the picking, --max-dets N bounds it.  Alongside --scales / --flip / --tiles it
runs over their forwards' candidates; alone the frame runs as a merge of ONE forward; with --vote the vote runs behind it.  No
reference script decays a score: there is no pin on the reference for it.

--matrix-nms linear|gaussian[:SIGMA] runs Matrix NMS (Wang et al., SOLOv2, 2020) in that place instead (Net.set_matrix_nms, once per
run): every candidate's score is decayed by its worst overlap with a higher-ranked candidate, compensated by that candidate's own
worst overlap -- no pick loop, so its cost does not grow with the detections that come out.  --soft-thr T and --max-dets N serve
whichever of the two is on; the flag is refused together with --soft-nms; alone it runs the frame as a merge of ONE forward.  These
are not Soft-NMS's scores (a decay is the worst single pair, compensated, not a product over picks), there is no pin on the
reference for it, and its accuracy against Soft-NMS was not evaluated (no labels here).

--wbf [THR] (default 0.55) runs weighted boxes fusion (Solovyev, Wang, Gabruseva, 2019 / 2021) in that place instead (Net.set_wbf,
once per run): the candidates are walked in score order into clusters -- a candidate joins the cluster whose fused box it overlaps
most, above THR --, a cluster's box is the score-weighted mean of ALL its members and its confidence their mean score (--wbf-conf
max: the largest) times min(members, N) / N, N = the forwards that looked at the frame (--wbf-expected N: another number; default 0
counts the views added), so an object one view out of four found is marked down.  --wbf-skip T (default 0) keeps candidates with a
score below T out, --max-dets N bounds the output.  Refused together with --soft-nms, --matrix-nms and --vote (a vote behind a fusion
would average twice); alone it runs the frame as a merge of ONE forward.  The result files are unchanged (the member counts are not
written).  There is no pin on the reference for it, and its accuracy against the other three was not evaluated (no labels here).

--seq-nms [avg|max] runs Seq-NMS (Han, Khorrami, Paine et al., 2016) over the frames of a stream (Net.set_seq_nms, once per run): the
input frames are taken --clip T (default 8) at a time in their order, the last clip may be shorter; one merge is opened per clip with T
lists per class, each forward of --batch B frames is added with list_of naming its frames' places in the clip, and the views of
--flip / --scales / --tiles go to their frame's list.  Per class, the boxes of neighbouring frames with an IoU above --seq-link THR
(default 0.5) are linked, the chain with the largest score sum comes out with its mean (avg, the default) or largest (max) score on
every box, and suppresses what its boxes overlap by more than --nms-overlap in their own frames.  --soft-thr T keeps candidates under
T out, --seq-top-k N (default 300, at most 1024) bounds the candidates of a frame and class, --max-dets N the output; --vote runs
behind it.  Refused together with --soft-nms, --matrix-nms and --wbf.  The result files keep their format; --tubelets-out DIR adds
DIR/<comp_id>_<class>.txt with rows [image_index sequence x y w h score], `sequence` unique within a clip and class.  No pin on the
reference, whose scripts run one forward per image and look at no other frame; accuracy was not evaluated (no labels here).

--track gives every detection a persistent track id across the frames of the run, which are taken as consecutive frames of one
stream in file order (Net.set_tracker, once per run): behind every final stage a table of tracks per class is stepped on the device
-- BYTE's two passes (Zhang et al., 2022): the detections with a score >= --track-high T (default 0.5) are associated first, IoU
above --track-match THR (default 0.3), then those >= --track-low T (default 0.1) with the tracks still unmatched; a constant-velocity
prediction of the centre (--track-motion linear, the default; none: the box stays) or, on request, the paper's Kalman filter
(--track-motion kalman: Net.set_tracker with motion none, then Net.set_tracker_kalman); as the matching a greedy walk by descending IoU
(--track-assign greedy, the default) or, on request, the optimal assignment the paper's solver finds (--track-assign optimal:
Net.set_tracker_assign; they differ where boxes overlap each other, and the optimal form costs a search per track).  The filter keeps (centre, aspect, height) and their velocities per track, with --track-kalman-pos S (default
0.05) and --track-kalman-vel S (default 0.00625) times the track's height as the standard deviations of position and velocity, and
--track-kalman-keep-height 1 (the default) freezing a lost track's height: use it where the detector's boxes jitter -- it smooths
the velocity and follows a change of size -- and not on clean, fast approaching boxes, where linear overlaps better.  An unmatched
detection over --track-high starts a track, a track lives through --track-max-age N missed frames (default 30) and shows its id
from its --track-min-hits N-th hit on (default 1).  Alone the
frames run in groups of one through Net.detect_multi; with --batch a group is B consecutive frames; with --scales / --flip / --tiles /
--vote / --soft-nms / --matrix-nms the tracker runs behind the frame's merge, with --seq-nms behind the clip's (the ids live on over
the clip boundary).  Refused together with --wbf, --rois-in and --proposals-only.  The result files are unchanged; --tracks-out DIR
adds DIR/<comp_id>_<class>.txt with rows [image_index track x y w h score], track 0 = no confirmed track.
--render-out DIR draws every frame's detections into a copy of the frame on the device (Net.render behind the frame's detect call:
the `show` block at the end of the reference scripts) and writes DIR/<frame>.png: every box with a score >= --show-thr T (the
scripts' show_thr: 0.3, and 0.1 for a Caltech model) outlined in its class's colour with --render-label score (the default: the
scripts print the score at the top edge), id or both (the track id; these need --track) or none; --render-color id colours by track
id (with --track); --pixelate N replaces every box's interior with an N x N mosaic (2 .. 64: anonymise the face nets' detections).
It works with --batch, --streams, --track and the merge flags; without one of them the frames go through detect_multi in groups of
one (Net.render reads the pack of a multi call).  The result files are unchanged.
--crops-out DIR hands every detection to a second stage as a patch: behind the frame's detect call, next to the render call,
Net.crops cuts the window of every box with a score >= --crop-thr T (default: the threshold above) out of the frame on the device and
resizes it to --crop-size HxW (default 128x64, the scripts' imresize); the window is the box scaled about its centre by
--crop-context F (default 1), with --crop-fit grown to the patch's aspect ratio instead of stretched, clipped to the frame or with
--crop-border shift moved inwards; --crop-min N drops windows under N pixels.  Every patch is written as DIR/<frame>_<slot>_<row>.png
(slot = the class's place in --cls-ids, row = the detection's place in its list, 0 = the best score), with --track as
DIR/id<track>/<frame>_<slot>_<row>.png -- a gallery per track; --crop-tracked (with --track) keeps confirmed tracks only.  The patch
is cut with mean 0, its planes reordered to RGB and every value v written as uint8(min(max(floor(v + .5), 0), 255)).  It works with
--batch, --streams, --track, the merge flags and --render-out, and is refused where --render-out is.  The result files are unchanged.
--streams N (with --track): the input is N cameras multiplexed, frame i of the input order (0-based) belongs to stream i % N, and
every stream has a table of tracks of its own (Net.set_tracker(streams=N); Net.set_frame_streams before every forward, from the
frames' own indices, so --batch B need not be a multiple of N).  One launch steps all the streams of a forward side by side.  Not with
--seq-nms (a clip is one stream).  --tracks-out then writes one file per stream, DIR/<comp_id>_<class>_stream<s>.txt, with the rows
and the 1-based image index that stream alone would have.  No pin on the reference,
whose scripts look at no other frame; accuracy was not evaluated (no labels here).

Everything here is host glue over calls the test-suite covers one by one (Net.set_image / set_images / set_image_views, forward,
detect / detect_multi, detect_merge_*, proposals_multi, kitti.write_*)."""
import argparse
import glob
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

KITTI_NAMES = {"car": ["bg", "car", "van", "truck", "tram"], "ped_cyc": ["bg", "ped", "cyc"], "caltech": ["bg", "ped"]}


def list_images(image_dir, limit=0):
    """dir([image_dir '*.png']) order (:29): by name; jpg accepted as well for the Caltech / CityPersons frames."""
    files = sorted(f for ext in ("png", "jpg", "jpeg") for f in glob.glob(os.path.join(image_dir, "*." + ext)))
    return files[:limit] if limit > 0 else files


def load_rgb_u8(path):
    """imread: H x W x 3 uint8 RGB (grey images are replicated like MATLAB users do before the [3 2 1] permutation)."""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))


def frame_id(path, k):
    """KITTI frame number of an image file (000123.png -> 123: what ImageSets/*.txt lists and writeLabels names the file after);
    the 0-based position for files that are not numbered."""
    stem = os.path.splitext(os.path.basename(path))[0] if path else ""
    return int(stem) if stem.isdigit() else k - 1


def load_frame(path, k):
    """Frame k (1-based) of the run: the file, or a frame of KITTI's size from the seeded generator (uint8 RGB, HWC)."""
    if path is None:
        rng = np.random.default_rng(1701 + k)
        return np.ascontiguousarray(rng.integers(0, 256, (375, 1242, 3), dtype=np.uint8))
    return load_rgb_u8(path)


def names_for(prototxt_text, names_arg):
    """Class names: --names, else from the width of cls_pred (5 = KITTI car nets, 3 = ped / cyc, 2 = pedestrian nets)."""
    if names_arg:
        return names_arg.split(",")
    import re
    m = re.search(r'name:\s*"cls_pred".*?num_output:\s*(\d+)', prototxt_text, re.S)
    n = int(m.group(1)) if m else 5
    return {5: KITTI_NAMES["car"], 3: KITTI_NAMES["ped_cyc"], 2: KITTI_NAMES["caltech"]}.get(n, ["bg"] + [f"class{i}" for i in range(1, n)])


def parse_scales(text):
    """--scales H1xW1,H2xW2,... -> [(H1, W1), (H2, W2), ...]; raises ValueError on anything else."""
    import re
    out = []
    for part in text.split(","):
        m = re.fullmatch(r"(\d+)x(\d+)", part.strip())
        if not m or int(m.group(1)) < 1 or int(m.group(2)) < 1:
            raise ValueError(f"--scales {text!r}: {part!r} is not HxW with positive integers")
        out.append((int(m.group(1)), int(m.group(2))))
    return out


def parse_tiles(text):
    """--tiles RxC[:overlap_px] -> (R, C, overlap); raises ValueError on anything else."""
    import re
    m = re.fullmatch(r"(\d+)x(\d+)(?::(\d+))?", text.strip())
    if not m or int(m.group(1)) < 1 or int(m.group(2)) < 1:
        raise ValueError(f"--tiles {text!r} is not RxC or RxC:overlap with positive R, C and an overlap >= 0")
    return int(m.group(1)), int(m.group(2)), int(m.group(3) or 0)


def add_merge_flags(ap):
    """The flags both drivers share for several forwards per frame (Net.detect_merge_*)."""
    ap.add_argument("--scales", default=None, help="H1xW1,H2xW2,...: run every frame at each of these net input sizes and merge the "
                    "candidates of all forwards before one NMS (Net.detect_merge_*)")
    ap.add_argument("--flip", action="store_true", help="also run every frame mirrored ([:, ::-1]) and merge its candidates in")
    ap.add_argument("--merge-cap", type=int, default=0, help="candidate slots per class and frame (default: forwards per frame x "
                    "BoxOutput's max_nms_num)")
    ap.add_argument("--tiles", default=None, help="RxC[:overlap_px]: cut every frame into R x C equal, overlapping windows, run each "
                    "as a view (Net.set_image_views) and merge their candidates before one NMS")
    ap.add_argument("--views-batch", action="store_true", help="with --flip and/or --tiles: all views of a frame as the images of ONE "
                    "forward (one set_image_views, one forward, one detect_merge_add(..., list_of=))")
    ap.add_argument("--vote", nargs="?", type=float, const=0.5, default=None, metavar="THR", help="box voting behind the merged NMS "
                    "(Net.set_box_voting): every kept box becomes the score-weighted mean of the candidates whose IoU with it is >= THR "
                    "(default 0.5); without --scales / --flip / --tiles the frame runs as a merge of one forward")
    ap.add_argument("--soft-nms", default=None, metavar="linear|gaussian[:SIGMA]", help="Soft-NMS in place of the merged hard NMS "
                    "(Net.set_soft_nms): a candidate that overlaps a picked box keeps living with a decayed score -- linear: by 1 - IoU above "
                    "--nms-overlap; gaussian: by exp(-IoU^2 / SIGMA), SIGMA default 0.5; without --scales / --flip / --tiles the frame runs "
                    "as a merge of one forward")
    ap.add_argument("--matrix-nms", default=None, metavar="linear|gaussian[:SIGMA]", help="Matrix NMS in place of the merged hard NMS "
                    "(Net.set_matrix_nms): every score decayed by its worst compensated overlap with a higher-ranked candidate, no pick "
                    "loop -- linear: min (1 - IoU) / (1 - comp); gaussian: exp(-max (IoU^2 - comp^2) / SIGMA), SIGMA default 0.5; not with "
                    "--soft-nms; without --scales / --flip / --tiles the frame runs as a merge of one forward")
    ap.add_argument("--wbf", nargs="?", type=float, const=0.55, default=None, metavar="THR", help="weighted boxes fusion in place of the merged "
                    "hard NMS (Net.set_wbf): candidates walked in score order into clusters (IoU with the cluster's fused box > THR, default "
                    "0.55), a cluster's box the score-weighted mean of its members, its confidence scaled by min(members, N) / N; not with "
                    "--soft-nms / --matrix-nms / --vote; without --scales / --flip / --tiles the frame runs as a merge of one forward")
    ap.add_argument("--wbf-skip", type=float, default=0.0, metavar="T", help="with --wbf: candidates with a score below T do not enter (default 0)")
    ap.add_argument("--wbf-conf", choices=["avg", "max"], default="avg", help="with --wbf: a cluster's confidence is its members' mean (avg, the "
                    "default) or largest (max) score")
    ap.add_argument("--wbf-expected", type=int, default=0, metavar="N", help="with --wbf: the N of min(members, N) / N (default 0: the views "
                    "added to the frame)")
    ap.add_argument("--seq-nms", nargs="?", const="avg", default=None, choices=["avg", "max"], help="Seq-NMS over clips of --clip frames in "
                    "place of the per-frame NMS (Net.set_seq_nms): the boxes of neighbouring frames are linked by IoU, the chain with the largest "
                    "score sum comes out with its mean (avg) or largest (max) score and suppresses what it overlaps; not with --soft-nms / "
                    "--matrix-nms / --wbf; --batch B frames share a forward")
    ap.add_argument("--clip", type=int, default=8, metavar="T", help="with --seq-nms: frames per clip, 1 .. 256 (default 8; the last clip may be "
                    "shorter)")
    ap.add_argument("--seq-link", type=float, default=0.5, metavar="THR", help="with --seq-nms: boxes of neighbouring frames with an IoU above THR "
                    "are linked (default 0.5)")
    ap.add_argument("--seq-top-k", type=int, default=300, metavar="N", help="with --seq-nms: at most N candidates per frame and class take part, "
                    "1 .. 1024 (default 300)")
    ap.add_argument("--tubelets-out", default=None, metavar="DIR", help="with --seq-nms: DIR/<comp_id>_<class>.txt with rows [image_index sequence "
                    "x y w h score]; sequence is unique within a clip and class")
    ap.add_argument("--track", action="store_true", help="track ids across the frames of the run (Net.set_tracker): BYTE association on the "
                    "device behind every final stage -- the frames are taken as consecutive frames of one stream, in file order; alone, with "
                    "--batch, --seq-nms, --scales, --flip, --tiles, --vote, --soft-nms and --matrix-nms; not with --wbf.  The result files are unchanged")
    ap.add_argument("--track-high", type=float, default=0.5, metavar="T", help="with --track: detections with a score >= T are associated first and "
                    "may start a track (default 0.5)")
    ap.add_argument("--track-low", type=float, default=0.1, metavar="T", help="with --track: detections with a score >= T (and below --track-high) are "
                    "offered to the tracks the first pass left unmatched (default 0.1)")
    ap.add_argument("--track-match", type=float, default=0.3, metavar="THR", help="with --track: a detection matches a track when their IoU is above "
                    "THR (default 0.3)")
    ap.add_argument("--track-motion", choices=["none", "linear", "kalman"], default="linear", help="with --track: a track's box stays where it was "
                    "seen (none), moves on with its smoothed centre velocity (linear, the default), or follows a Kalman filter on centre, "
                    "aspect and height (kalman: Net.set_tracker_kalman; for jittering boxes, not for clean fast approaching ones)")
    ap.add_argument("--track-kalman-pos", type=float, default=1 / 20, metavar="S", help="with --track-motion kalman: the standard deviation of a "
                    "position, times the track's height (default 0.05)")
    ap.add_argument("--track-kalman-vel", type=float, default=1 / 160, metavar="S", help="with --track-motion kalman: the standard deviation of a "
                    "velocity, times the track's height (default 0.00625)")
    ap.add_argument("--track-kalman-keep-height", type=int, choices=[0, 1], default=1, metavar="0|1", help="with --track-motion kalman: a track that "
                    "missed a frame keeps its height (1, the default) or goes on changing it (0)")
    ap.add_argument("--track-assign", choices=["greedy", "optimal"], default="greedy", help="with --track: the matching of both passes is the walk "
                    "by descending IoU (greedy, the default) or the maximum-weight assignment (optimal: Net.set_tracker_assign; keeps ids "
                    "the walk loses where boxes overlap each other)")
    ap.add_argument("--track-max-age", type=int, default=30, metavar="N", help="with --track: a track lives through N missed frames (default 30)")
    ap.add_argument("--track-min-hits", type=int, default=1, metavar="N", help="with --track: a track shows its id from its N-th hit on (default 1)")
    ap.add_argument("--streams", type=int, default=1, metavar="N", help="with --track: the frames are N multiplexed cameras, frame i of the "
                    "input order belongs to stream i %% N and every stream has its own tracks (Net.set_tracker(streams=N), "
                    "Net.set_frame_streams per forward); --tracks-out writes one file per stream.  Not with --seq-nms")
    ap.add_argument("--tracks-out", default=None, metavar="DIR", help="with --track: DIR/<comp_id>_<class>.txt with rows [image_index track x y w h "
                    "score]; track 0 = no confirmed track")
    ap.add_argument("--render-out", default=None, metavar="DIR", help="draw every frame's detections into a copy of the frame on the device "
                    "(Net.render) and write DIR/<frame>.png")
    ap.add_argument("--show-thr", type=float, default=None, metavar="T", help="with --render-out: draw the boxes with a score >= T (default: the "
                    "scripts' show_thr, 0.3, and 0.1 for a Caltech model)")
    ap.add_argument("--render-label", choices=["none", "score", "id", "both"], default="score", help="with --render-out: what is printed at a "
                    "box's top edge (default score, as the scripts; id and both need --track)")
    ap.add_argument("--render-color", choices=["slot", "id"], default="slot", help="with --render-out: a colour per class (slot, the default) "
                    "or per track id (needs --track)")
    ap.add_argument("--pixelate", type=int, default=0, metavar="N", help="with --render-out: replace every drawn box's interior with an N x N "
                    "mosaic of the frame, 2 .. 64 (default 0: off)")
    ap.add_argument("--crops-out", default=None, metavar="DIR", help="cut every detection out of its frame on the device as a fixed-size patch "
                    "(Net.crops) and write DIR/<frame>_<slot>_<row>.png, with --track DIR/id<track>/<frame>_<slot>_<row>.png")
    ap.add_argument("--crop-size", default="128x64", metavar="HxW", help="with --crops-out: the patch size, each 1 .. 1024 (default 128x64)")
    ap.add_argument("--crop-thr", type=float, default=None, metavar="T", help="with --crops-out: cut the boxes with a score >= T (default: the "
                    "threshold --render-out draws with)")
    ap.add_argument("--crop-context", type=float, default=1.0, metavar="F", help="with --crops-out: the window is the box scaled about its centre "
                    "by F, 1 .. 16 (default 1)")
    ap.add_argument("--crop-fit", action="store_true", help="with --crops-out: grow the window to the patch's aspect ratio instead of stretching it")
    ap.add_argument("--crop-border", choices=["clip", "shift"], default="clip", help="with --crops-out: a window that leaves the frame is clipped "
                    "(the default) or moved inwards")
    ap.add_argument("--crop-min", type=int, default=1, metavar="N", help="with --crops-out: no patch of a window narrower or lower than N pixels "
                    "(default 1)")
    ap.add_argument("--crop-tracked", action="store_true", help="with --crops-out and --track: only the detections of a confirmed track")
    ap.add_argument("--soft-thr", type=float, default=0.001, metavar="T", help="with --soft-nms: stop picking when the best live score is below T; "
                    "with --matrix-nms: keep the scores >= T (default 0.001)")
    ap.add_argument("--max-dets", type=int, default=0, metavar="N", help="with --soft-nms / --matrix-nms / --wbf: at most N detections per class and "
                    "frame (default 0: no bound)")


def parse_soft_nms(text, flag="--soft-nms"):
    """'linear' | 'gaussian' | 'gaussian:SIGMA' -> (method, sigma)."""
    import re
    m = re.fullmatch(r"(linear|gaussian)(?::([^:]+))?", text.strip())
    try:
        sigma = float(m.group(2)) if m and m.group(2) else 0.5
    except ValueError:
        m = None
    if not m or (m.group(1) == "linear" and m.group(2)) or not 0.0 < sigma < float("inf"):
        raise ValueError(f"{flag} {text!r} is not linear, gaussian or gaussian:SIGMA with a finite SIGMA > 0")
    return m.group(1), sigma


def one_forward_merge(a):
    """--vote, --soft-nms, --matrix-nms and --wbf live in detect_merge_end: on their own they run the frame as a merge of one forward."""
    return a.vote is not None or a.soft_nms is not None or a.matrix_nms is not None or a.wbf is not None


def seq_on(a):
    """--seq-nms: the run goes clip by clip (run_seq_clips), whatever else is set."""
    return getattr(a, "seq_nms", None) is not None


def track_on(a):
    """--track: every final stage of the run steps the tracker (Net.set_tracker)."""
    return bool(getattr(a, "track", False))


def render_on(a):
    """--render-out: every detect call of the run is followed by a Net.render of its frames."""
    return getattr(a, "render_out", None) is not None


def show_thr_of(a):
    """--show-thr, or the scripts' show_thr: 0.1 in examples/caltech/run_mscnn_detection.m, 0.3 in the KITTI and WiderFace scripts."""
    if a.show_thr is not None:
        return a.show_thr
    return 0.1 if "caltech" in (getattr(a, "model", None) or getattr(a, "prototxt", None) or "").lower() else 0.3


def render_frames(net, a, frames, paths, first):
    """--render-out behind a detect_multi / detect_cascade_multi / detect_merge_end over `frames` (numpy arrays, or the device tensors
    the forward was fed from: then the frames never leave the device before they are drawn on): DIR/<frame>.png for each; `first` is
    the 1-based number of frames[0] in the run."""
    if not render_on(a):
        return
    from PIL import Image
    outs = net.render(frames, thr=show_thr_of(a), label=a.render_label, color_by=a.render_color, pixelate=a.pixelate)
    os.makedirs(a.render_out, exist_ok=True)
    for i, (o, path) in enumerate(zip(outs, paths)):
        arr = o if isinstance(o, np.ndarray) else o.cpu().numpy()
        Image.fromarray(arr, "RGB").save(os.path.join(a.render_out, f"{frame_id(path, first + i):06d}.png"))


def crops_on(a):
    """--crops-out: every detect call of the run is followed by a Net.crops of its frames."""
    return getattr(a, "crops_out", None) is not None


def crop_thr_of(a):
    """--crop-thr, or the threshold the `show` block would draw with (show_thr_of)."""
    return a.crop_thr if a.crop_thr is not None else show_thr_of(a)


def parse_crop_size(text):
    """--crop-size HxW -> (H, W), each 1 .. 1024; raises ValueError on anything else."""
    import re
    m = re.fullmatch(r"(\d+)x(\d+)", text.strip())
    if not m or not (1 <= int(m.group(1)) <= 1024 and 1 <= int(m.group(2)) <= 1024):
        raise ValueError(f"--crop-size {text!r} is not HxW with both inside 1 .. 1024")
    return int(m.group(1)), int(m.group(2))


def patch_to_rgb_u8(patch):
    """A float [3, h, w] patch of Net.crops with mean 0 (planes B, G, R) as a uint8 RGB image [h, w, 3]: every value v, in double,
    becomes uint8(min(max(floor(v + .5), 0), 255)) -- the bicubic resize overshoots, hence the clamp."""
    v = np.asarray(patch, np.float64)[::-1].transpose(1, 2, 0)
    return np.ascontiguousarray(np.minimum(np.maximum(np.floor(v + .5), 0), 255).astype(np.uint8))


def crop_frames(net, a, frames, paths, first):
    """--crops-out behind a detect_multi / detect_cascade_multi / detect_merge_end over `frames` (numpy arrays or device tensors, as
    render_frames): every detection with a score >= the threshold as DIR/<frame>_<slot>_<row>.png, with --track as
    DIR/id<track>/<frame>_<slot>_<row>.png (id0: no confirmed track); `first` is the 1-based number of frames[0] in the run."""
    if not crops_on(a):
        return
    from PIL import Image
    patches, info = net.crops(frames, size=a.crop_size, thr=crop_thr_of(a), context=a.crop_context, fit=a.crop_fit, border=a.crop_border,
                              min_size=a.crop_min, tracked_only=a.crop_tracked)
    arr = patches if isinstance(patches, np.ndarray) else patches.cpu().numpy()
    for patch, rec in zip(arr, info):
        b = int(rec["frame"])
        d = os.path.join(a.crops_out, f"id{int(rec['track_id'])}") if track_on(a) else a.crops_out
        os.makedirs(d, exist_ok=True)
        Image.fromarray(patch_to_rgb_u8(patch), "RGB").save(os.path.join(d, f"{frame_id(paths[b], first + b):06d}_{int(rec['slot'])}_{int(rec['row'])}.png"))


def apply_track_setting(net, a):
    """The sticky tracker setting of the run, once, before its first frame."""
    if track_on(a):
        kalman = a.track_motion == "kalman"
        net.set_tracker(high_thr=a.track_high, low_thr=a.track_low, match_thr=a.track_match, motion="none" if kalman else a.track_motion,
                        max_age=a.track_max_age, min_hits=a.track_min_hits, streams=a.streams)
        if kalman:      # (keeps the streams)
            net.set_tracker_kalman(std_position=a.track_kalman_pos, std_velocity=a.track_kalman_vel,
                                   freeze_lost_height=bool(a.track_kalman_keep_height))
        if a.track_assign != "greedy":
            net.set_tracker_assign(a.track_assign)


def set_group_streams(net, a, first, count):
    """--streams N: in front of a tracked call over the frames first .. first + count - 1 of the run (0-based), frame i is stream i % N."""
    if track_on(a) and a.streams > 1:
        net.set_frame_streams([(first + i) % a.streams for i in range(count)])


def write_tracks(path, per_frame_dets, per_frame_ids, streams=1):
    """--tracks-out: the file `path` (write_tubelets' rows); with --streams N > 1 one file per stream, `path` with _stream<s> in front of
    its extension, holding the frames of that stream numbered from 1.  Returns the paths written."""
    if streams <= 1:
        write_tubelets(path, per_frame_dets, per_frame_ids)
        return [path]
    stem, ext = os.path.splitext(path)
    out = []
    for s in range(streams):
        out.append(f"{stem}_stream{s}{ext}")
        write_tubelets(out[-1], per_frame_dets[s::streams], per_frame_ids[s::streams])
    return out


def frame_tracks(net, a):
    """Behind a detect call of the run: [[ids per slot] per frame of that call] with --track, else None."""
    return net.detect_tracks() if track_on(a) else None


def apply_merge_settings(net, a):
    """The sticky settings of every detect_merge_end of the run."""
    if a.vote is not None:
        net.set_box_voting(a.vote)
    if a.soft_nms is not None:
        net.set_soft_nms(a.soft_nms[0], sigma=a.soft_nms[1], score_thr=a.soft_thr, max_out=a.max_dets)
    if a.matrix_nms is not None:
        net.set_matrix_nms(a.matrix_nms[0], sigma=a.matrix_nms[1], score_thr=a.soft_thr, max_out=a.max_dets)
    if a.wbf is not None:
        net.set_wbf(a.wbf, skip_thr=a.wbf_skip, conf=a.wbf_conf, expected=a.wbf_expected, max_out=a.max_dets)
    if seq_on(a):
        net.set_seq_nms(a.seq_link, score_thr=a.soft_thr, top_k=a.seq_top_k, rescore=a.seq_nms, max_out=a.max_dets)


def check_merge_flags(ap, a):
    if a.scales is not None:
        try:
            a.scales = parse_scales(a.scales)
        except ValueError as e:
            ap.error(str(e))
    if a.tiles is not None:
        try:
            a.tiles = parse_tiles(a.tiles)
        except ValueError as e:
            ap.error(str(e))
    if a.views_batch and not (a.flip or a.tiles):
        ap.error("--views-batch batches the views of a frame: give --flip and/or --tiles")
    if a.vote is not None and not 0.0 < a.vote < 1.0:
        ap.error(f"--vote {a.vote:g}: the threshold must lie inside (0, 1)")
    if a.soft_nms is not None:
        try:
            a.soft_nms = parse_soft_nms(a.soft_nms)
        except ValueError as e:
            ap.error(str(e))
    if a.matrix_nms is not None:
        if a.soft_nms is not None:
            ap.error("--matrix-nms and --soft-nms exclude each other: one of them replaces the merged NMS")
        try:
            a.matrix_nms = parse_soft_nms(a.matrix_nms, "--matrix-nms")
        except ValueError as e:
            ap.error(str(e))
    if a.wbf is not None:
        for flag, on in (("--soft-nms", a.soft_nms is not None), ("--matrix-nms", a.matrix_nms is not None), ("--vote", a.vote is not None)):
            if on:
                ap.error(f"--wbf and {flag} exclude each other: the fusion replaces the merged NMS and averages the boxes itself")
        if not 0.0 < a.wbf < 1.0:
            ap.error(f"--wbf {a.wbf:g}: the threshold must lie inside (0, 1)")
        if not 0.0 <= a.wbf_skip < float("inf"):
            ap.error(f"--wbf-skip {a.wbf_skip:g}: the threshold must be a finite value >= 0")
        if a.wbf_expected < 0:
            ap.error(f"--wbf-expected {a.wbf_expected}: must be >= 0")
    elif a.wbf_skip != 0.0 or a.wbf_conf != "avg" or a.wbf_expected != 0:
        ap.error("--wbf-skip / --wbf-conf / --wbf-expected belong to --wbf")
    if seq_on(a):
        for flag, on in (("--soft-nms", a.soft_nms is not None), ("--matrix-nms", a.matrix_nms is not None), ("--wbf", a.wbf is not None)):
            if on:
                ap.error(f"--seq-nms and {flag} exclude each other: one of them replaces the merged NMS")
        if not 1 <= a.clip <= 256:
            ap.error(f"--clip {a.clip}: a clip has 1 .. 256 frames")
        if not 0.0 < a.seq_link < 1.0:
            ap.error(f"--seq-link {a.seq_link:g}: the threshold must lie inside (0, 1)")
        if not 1 <= a.seq_top_k <= 1024:
            ap.error(f"--seq-top-k {a.seq_top_k}: must be 1 .. 1024")
        if a.batch > 1 and (a.tiles or a.views_batch):
            ap.error("--seq-nms with --tiles / --views-batch runs one frame's views per forward (drop --batch)")
    elif a.clip != 8 or a.seq_link != 0.5 or a.seq_top_k != 300 or a.tubelets_out is not None:
        ap.error("--clip / --seq-link / --seq-top-k / --tubelets-out belong to --seq-nms")
    if track_on(a):
        if a.wbf is not None:
            ap.error("--track and --wbf exclude each other: the track ids come back where the fusion's member counts do")
        if not a.track_low <= a.track_high:      # (a NaN fails)
            ap.error(f"--track-low {a.track_low:g} must not be above --track-high {a.track_high:g}")
        if not 0.0 <= a.track_match < 1.0:
            ap.error(f"--track-match {a.track_match:g}: the threshold must lie inside [0, 1)")
        if a.track_max_age < 0 or a.track_min_hits < 1:
            ap.error(f"--track-max-age {a.track_max_age} must be >= 0, --track-min-hits {a.track_min_hits} >= 1")
        if not 1 <= a.streams <= 256:
            ap.error(f"--streams {a.streams}: 1 .. 256 streams")
        if a.track_motion == "kalman":
            if not (0.0 < a.track_kalman_pos < float("inf") and 0.0 < a.track_kalman_vel < float("inf")):      # (a NaN fails)
                ap.error(f"--track-kalman-pos {a.track_kalman_pos:g} and --track-kalman-vel {a.track_kalman_vel:g} must be finite and above 0")
        elif a.track_kalman_pos != 1 / 20 or a.track_kalman_vel != 1 / 160 or a.track_kalman_keep_height != 1:
            ap.error("--track-kalman-pos / --track-kalman-vel / --track-kalman-keep-height belong to --track-motion kalman")
        if a.streams > 1 and seq_on(a):
            ap.error(f"--streams {a.streams} and --seq-nms exclude each other: a clip links every frame to the one before it, so it is one stream")
    elif a.streams != 1:
        ap.error(f"--streams {a.streams} belongs to --track")
    elif (a.track_high != 0.5 or a.track_low != 0.1 or a.track_match != 0.3 or a.track_motion != "linear" or a.track_max_age != 30
          or a.track_min_hits != 1 or a.tracks_out is not None or a.track_kalman_pos != 1 / 20 or a.track_kalman_vel != 1 / 160
          or a.track_kalman_keep_height != 1 or a.track_assign != "greedy"):
        ap.error("--track-high / --track-low / --track-match / --track-motion / --track-max-age / --track-min-hits / --track-kalman-pos / "
                 "--track-kalman-vel / --track-kalman-keep-height / --track-assign / --tracks-out belong to --track")
    if render_on(a):
        if a.render_label in ("id", "both") and not track_on(a):
            ap.error(f"--render-label {a.render_label} prints the track id: it needs --track")
        if a.render_color == "id" and not track_on(a):
            ap.error("--render-color id colours by track id: it needs --track")
        if a.pixelate != 0 and not 2 <= a.pixelate <= 64:
            ap.error(f"--pixelate {a.pixelate}: the mosaic's block edge, 2 .. 64 (0: off)")
        if a.show_thr is not None and a.show_thr != a.show_thr:
            ap.error("--show-thr nan: the threshold must be a number")
        if getattr(a, "rois_in", "") or getattr(a, "proposals_only", False):
            ap.error("--render-out draws the detections of every frame: not with --rois-in (frames without a box run no final stage) or "
                     "--proposals-only")
    elif a.show_thr is not None or a.render_label != "score" or a.render_color != "slot" or a.pixelate != 0:
        ap.error("--show-thr / --render-label / --render-color / --pixelate belong to --render-out")
    if crops_on(a):
        try:
            a.crop_size = parse_crop_size(a.crop_size)
        except ValueError as e:
            ap.error(str(e))
        if a.crop_thr is not None and a.crop_thr != a.crop_thr:
            ap.error("--crop-thr nan: the threshold must be a number")
        if not 1.0 <= a.crop_context <= 16.0:      # (a NaN fails)
            ap.error(f"--crop-context {a.crop_context:g}: the factor must lie inside [1, 16]")
        if a.crop_min < 1:
            ap.error(f"--crop-min {a.crop_min}: must be >= 1")
        if a.crop_tracked and not track_on(a):
            ap.error("--crop-tracked keeps the detections of confirmed tracks: it needs --track")
        if getattr(a, "rois_in", "") or getattr(a, "proposals_only", False):
            ap.error("--crops-out cuts the detections of every frame: not with --rois-in (frames without a box run no final stage) or "
                     "--proposals-only")
    elif (a.crop_size != "128x64" or a.crop_thr is not None or a.crop_context != 1.0 or a.crop_fit or a.crop_border != "clip" or a.crop_min != 1
          or a.crop_tracked):
        ap.error("--crop-size / --crop-thr / --crop-context / --crop-fit / --crop-border / --crop-min / --crop-tracked belong to --crops-out")
    if not 0.0 <= a.soft_thr < float("inf"):
        ap.error(f"--soft-thr {a.soft_thr:g}: the threshold must be a finite value >= 0")
    if a.max_dets < 0:
        ap.error(f"--max-dets {a.max_dets}: must be >= 0")
    if a.soft_nms is None and a.matrix_nms is None and not seq_on(a) and (a.soft_thr != 0.001 or (a.max_dets != 0 and a.wbf is None)):
        ap.error("--soft-thr belongs to --soft-nms, --matrix-nms or --seq-nms, --max-dets to one of them or to --wbf")
    if (a.scales or a.flip or a.tiles or one_forward_merge(a)) and a.batch > 1 and not seq_on(a):
        ap.error("--scales / --flip / --tiles / --vote / --soft-nms / --matrix-nms / --wbf run one frame per forward (drop --batch; --views-batch batches a frame's "
                 "views)")


def merge_cand_cap(prototxt_text, passes, merge_cap):
    """Slots of a candidate list: --merge-cap, else forwards per frame x the largest max_nms_num of the deploy (BoxOutput's row bound
    of one forward of one frame)."""
    import re
    if merge_cap > 0:
        return merge_cap
    bounds = [int(v) for v in re.findall(r"max_nms_num:\s*(\d+)", prototxt_text)]
    if not bounds or max(bounds) < 1:
        sys.exit("--scales / --flip: the deploy has no max_nms_num > 0 to size the candidate lists by: give --merge-cap N")
    return passes * max(bounds)


def merge_passes(a, net_hw):
    """[(H, W, flipped)] of the forwards of one frame, in add order: every scale, each followed by its mirrored twin."""
    return [(H, W, f) for H, W in (a.scales or [net_hw]) for f in ((False, True) if a.flip else (False,))]


def frame_views(a, org_hw):
    """--tiles / --views-batch: (views, merge views) of one frame -- its tiles, or the whole frame, with --flip the mirrors behind them."""
    from mscnn_amd import net as mnet
    rows, cols, overlap = a.tiles or (1, 1, 0)
    views, _, mviews = mnet.tile_views(org_hw, rows, cols, overlap=overlap, flip=a.flip)
    return views, mviews


def views_per_frame(a):
    rows, cols, _ = a.tiles or (1, 1, 0)
    return rows * cols * (2 if a.flip else 1)


def run_frame_views(a, net, img, scales, shape, add):
    """--tiles / --views-batch for ONE frame between detect_merge_begin and _end: per input size either one batched forward over all
    views (--views-batch) or one forward per view, each straight out of the frame uploaded here once (Net.set_image_views).
    add(params, merge views, list_of or None) is the driver's detect_merge_add.  Returns (the input's shape now, seconds in forwards)."""
    import torch
    views, mviews = frame_views(a, img.shape[:2])
    dev_img = torch.from_numpy(img).cuda(a.device)                            # (kept referenced until the pre-processing has run)
    groups = [list(range(len(views)))] if a.views_batch else [[v] for v in range(len(views))]
    used = 0.0
    for H, W in scales:
        for g in groups:
            if (len(g), 3, H, W) != tuple(shape):
                shape = (len(g), 3, H, W)
                net.reshape_input("data", shape)
            params = net.set_image_views("data", [dev_img], [views[v] for v in g])
            torch.cuda.synchronize(a.device)
            t0 = time.perf_counter()
            net.forward()
            torch.cuda.synchronize(a.device)
            used += time.perf_counter() - t0                                  # forwards only, as :72-73
            add(params, [mviews[v] for v in g], [0] * len(g) if a.views_batch else None)
    return shape, used


def run_seq_clips(a, net, text, files, net_hw, shape, slots, load, add):
    """--seq-nms for both drivers: the frames --clip T at a time; per clip one detect_merge_begin with T lists per slot, per input size
    (and mirror) one forward per --batch B frames of the clip, added with list_of = the frames' places in the clip -- with --tiles /
    --views-batch the views of every frame, to that frame's list --, one detect_merge_end and its detect_merge_sequences.
    add(params, merge views or None, list_of) is the driver's detect_merge_add.  Returns (per frame of the run ([dets per slot],
    [sequence ids per slot], [track ids per slot] or None without --track), the input's shape now, seconds in forwards)."""
    import torch
    passes = merge_passes(a, net_hw)
    by_views = bool(a.tiles or a.views_batch)
    n_fwd = len(a.scales or [0]) * views_per_frame(a) if by_views else len(passes)
    cand_cap = merge_cand_cap(text, n_fwd, a.merge_cap)
    apply_merge_settings(net, a)                                              # sticky: every detect_merge_end below runs Seq-NMS
    out, used = [], 0.0
    for c0 in range(0, len(files), a.clip):
        imgs = [load(path, c0 + i + 1) for i, path in enumerate(files[c0:c0 + a.clip])]
        net.detect_merge_begin(len(imgs), slots, cand_cap)
        for t, img in enumerate(imgs if by_views else []):
            shape, dt = run_frame_views(a, net, img, a.scales or [tuple(net_hw)], shape, lambda p, mv, lo, t=t: add(p, mv, [t] * len(p)))
            used += dt
        for H, W, flipped in () if by_views else passes:
            for g0 in range(0, len(imgs), a.batch):
                group = imgs[g0:g0 + a.batch]
                if (len(group), 3, H, W) != tuple(shape):
                    shape = (len(group), 3, H, W)
                    net.reshape_input("data", shape)
                dev_imgs = [torch.from_numpy(np.ascontiguousarray(f[:, ::-1]) if flipped else f).cuda(a.device) for f in group]
                params = net.set_images("data", dev_imgs)
                torch.cuda.synchronize(a.device)
                t0 = time.perf_counter()
                net.forward()
                torch.cuda.synchronize(a.device)
                used += time.perf_counter() - t0                              # forwards only, as :72-73
                add(params, [dict(flip_x=1)] * len(group) if flipped else None, list(range(g0, g0 + len(group))))
        per_image, _ = net.detect_merge_end()
        seqs = net.detect_merge_sequences()
        trks = frame_tracks(net, a)
        render_frames(net, a, imgs, files[c0:c0 + a.clip], c0 + 1)
        crop_frames(net, a, imgs, files[c0:c0 + a.clip], c0 + 1)
        out += [([per_image[t][s][0] for s in range(slots)], [seqs[t][s] for s in range(slots)], trks[t] if trks else None) for t in range(len(imgs))]
        k = c0 + len(imgs)
        print(f"idx {k}/{len(files)}, avgtime={used / k:.4f}s (clips of {a.clip} frames, {n_fwd} forwards per frame)")
    return out, shape, used


def write_tubelets(path, per_frame_dets, per_frame_seq):
    """--tubelets-out, and --tracks-out with the track ids: rows [image_index sequence x y w h score] (1-based index, %.5g as the result
    files) of one class."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for i, (dets, seq) in enumerate(zip(per_frame_dets, per_frame_seq), start=1):
            for d, q in zip(dets, seq):
                f.write(",".join(["%.5g" % float(v) for v in [i, q] + list(d[:5])]) + "\n")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--prototxt"); ap.add_argument("--weights", help=".caffemodel (new or V1 layout) or .h5 snapshot")
    ap.add_argument("--model", help="a deploy net of mscnn_amd.zoo instead of --prototxt (e.g. kitti_car/mscnn-7s-576)")
    ap.add_argument("--images", help="directory of *.png / *.jpg frames")
    ap.add_argument("--synthetic", type=int, default=0, help="N synthetic KITTI-shaped frames instead of --images")
    ap.add_argument("--out", default="detections"); ap.add_argument("--comp-id", default="mscnn_mi355x")
    ap.add_argument("--cls-ids", default="2", help="1-based class columns, comma separated (the reference's cls_ids)")
    ap.add_argument("--names", default=""); ap.add_argument("--labels-dir", default="")
    ap.add_argument("--precision", default="f32", choices=["f32", "f16x3", "f16"])
    ap.add_argument("--proposal-thr", type=float, default=-10.0); ap.add_argument("--nms-overlap", type=float, default=0.5)
    ap.add_argument("--limit", type=int, default=0); ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--batch", type=int, default=1, help="frames per forward (> 1: Net.set_images + one detect_multi per group)")
    ap.add_argument("--nms-type", default="maxg", choices=["maxg", "max"], help="pNms.type (bbNms.m: greedy or not)")
    ap.add_argument("--ovr-dnm", default="union", choices=["union", "min"], help="pNms.ovrDnm: the overlap's denominator")
    ap.add_argument("--nms-thr", type=float, default=None, help="bbNms's thr: drop rows with prob <= this before the NMS (default -inf)")
    ap.add_argument("--det-thr", type=float, default=0.0, help="> 0: drop rows under this probability before the NMS "
                    "(widerface/run_mscnn_detection.m:139-143)")
    ap.add_argument("--proposals-out", default="", help="directory for <comp_id>.txt: rows [image_index x y w h score] of every image's "
                    "filtered, rescaled proposals (final_proposals of the scripts)")
    ap.add_argument("--proposals-only", action="store_true", help="run the net up to BoxOutput only (Net.forward_proposals): no detect "
                    "call, no detection files; needs --proposals-out")
    ap.add_argument("--rois-in", default="", help="file of rows [image_index x y w h score] (1-based index, original-image pixels: what "
                    "--proposals-out writes): run the detection sub-net on these boxes (Net.forward_rois) instead of the whole net")
    add_merge_flags(ap)
    a = ap.parse_args(argv)
    check_merge_flags(ap, a)
    if (a.scales or a.flip or a.tiles or one_forward_merge(a) or seq_on(a)) and (a.rois_in or a.proposals_out or a.proposals_only):
        ap.error("--scales / --flip / --tiles / --vote / --soft-nms / --matrix-nms merge detections: not with --rois-in, --proposals-out or --proposals-only")
    if track_on(a) and (a.rois_in or a.proposals_only):
        ap.error("--track follows the detections of every frame: not with --rois-in (frames without a box run no final stage) or --proposals-only")
    if a.proposals_only and not a.proposals_out:
        ap.error("--proposals-only needs --proposals-out DIR")
    if a.proposals_only and a.rois_in:
        ap.error("--rois-in runs the detection sub-net on given boxes, --proposals-only stops in front of it: not both")
    if not (a.prototxt or a.model) or not (a.images or a.synthetic):
        ap.error("need --prototxt or --model, and --images or --synthetic N")
    return a


def read_rois(path, n_frames):
    """--rois-in: the file's rows [image_index x y w h score] (1-based index, ascending: the layout of --proposals-out) as one float64
    array [n, 5] = [x y w h score] per frame of the run; a frame the file does not mention has 0 rows."""
    from mscnn_amd import kitti
    per_frame = [[] for _ in range(n_frames)]
    prev = 1
    for ln, row in enumerate(kitti.read_detections_dlm(path), start=1):
        if len(row) != 6:
            raise ValueError(f"{path}: row {ln} has {len(row)} values, not [image_index x y w h score]")
        k = int(row[0])
        if k != row[0] or k < 1 or k > n_frames:
            raise ValueError(f"{path}: row {ln}: image index {row[0]:g} outside 1 .. {n_frames}")
        if k < prev:
            raise ValueError(f"{path}: row {ln}: image index {k} after {prev}: rows must be grouped by image in ascending order")
        prev = k
        per_frame[k - 1].append(row[1:])
    return [np.asarray(r, np.float64).reshape(-1, 5) for r in per_frame]


def group_rois(per_frame):
    """The frames of one forward -> forward_rois' "image" rows [R, 6] float64 with the 0-based index inside the group."""
    return np.concatenate([np.concatenate([np.full((len(r), 1), float(i)), r], axis=1) for i, r in enumerate(per_frame)], axis=0)


def main(argv=None):
    a = parse_args(argv)

    import torch
    from mscnn_amd import kitti, net as mnet, synth, zoo
    text = open(a.prototxt).read() if a.prototxt else zoo.prototxt(a.model)
    net = mnet.Net(prototxt_text=text, device=a.device)
    net.set_nms(type=a.nms_type, ovr_dnm=a.ovr_dnm, thr=a.nms_thr, det_thr=a.det_thr)      # sticky, like pNms at the top of the script
    if a.weights:
        net.load_caffemodel(a.weights)              # net.cpp:788-795: ".h5" -> HDF5 snapshot, else binary NetParameter
    else:
        print("no --weights: seeded He-normal weights (synth.load_into) -- detections are meaningless, timings are not", file=sys.stderr)
        synth.load_into(net, "mid")
    if a.precision != "f32":
        net.set_precision(a.precision)
    imgH, imgW = net.blob_shape("data")[2:]
    names = names_for(text, a.names)
    cls_ids = [int(c) for c in a.cls_ids.split(",")]
    files = list_images(a.images, a.limit) if a.images else [None] * a.synthetic
    if not files:
        sys.exit(f"no images in {a.images}")
    if a.batch < 1:
        ap.error("--batch must be >= 1")
    per_class = {c: [] for c in cls_ids}
    per_image_props = []
    forward = net.forward_proposals if a.proposals_only else net.forward
    rois = read_rois(a.rois_in, len(files)) if a.rois_in else None
    apply_track_setting(net, a)
    a.track_ids = []                                                          # --track: per frame of the run [ids per class]
    if seq_on(a):
        return run_seq(a, net, text, files, names, cls_ids, imgH, imgW, per_class)
    if a.batch > 1:
        return run_batched(a, net, files, names, cls_ids, imgH, imgW, per_class, per_image_props, forward, rois)
    if a.scales or a.flip or a.tiles or one_forward_merge(a):
        return run_merged(a, net, text, files, names, cls_ids, imgH, imgW, per_class)
    if track_on(a) or render_on(a) or crops_on(a):                            # --track / --render-out / --crops-out alone: groups of one frame through detect_multi
        return run_batched(a, net, files, names, cls_ids, imgH, imgW, per_class, per_image_props, forward, rois)      # (Net.detect is refused while the tracker is on, and leaves Net.render / Net.crops no pack)
    used = 0.0
    for k, path in enumerate(files, start=1):
        img = load_frame(path, k)
        orgH, orgW = img.shape[:2]
        ratios = (imgH / float(orgH), imgW / float(orgW))                      # :63
        dev_img = torch.from_numpy(img).cuda(a.device)                       # (kept referenced until the pre-processing has run)
        net.set_image("data", dev_img)                                       # :64-69 on the device
        torch.cuda.synchronize(a.device)
        t0 = time.perf_counter()
        ran = True
        if rois is None:
            forward()
        elif len(rois[k - 1]):
            net.forward_rois(group_rois([rois[k - 1]]), "image", [dict(ratios=ratios)])
        else:
            ran = False                                                       # no box for this frame: nothing to run, no detections
        torch.cuda.synchronize(a.device)
        used += time.perf_counter() - t0                                      # :72-73: forward only
        if a.proposals_out:                                                   # :75-91
            per_image_props.append(net.proposals_multi([dict(ratios=ratios, proposal_thr=a.proposal_thr)])[0][0][0] if ran
                                   else np.zeros((0, 5)))
        by_type = {}
        for c in () if a.proposals_only else cls_ids:
            dets = np.zeros((0, 5))
            if ran:
                dets, _, _ = net.detect(cls_id=c, ratios=ratios, org_hw=(orgH, orgW), proposal_thr=a.proposal_thr, nms_overlap=a.nms_overlap)
            per_class[c].append(dets)
            by_type[{"car": "Car", "ped": "Pedestrian", "cyc": "Cyclist"}.get(names[c - 1], names[c - 1])] = dets
        if a.labels_dir and not a.proposals_only:                             # writeDetForEval.m:88-89: the frame's own KITTI id
            kitti.write_kitti_labels(a.labels_dir, frame_id(path, k), by_type)
        if k % 100 == 0 or k == len(files):
            print(f"idx {k}/{len(files)}, avgtime={used / k:.4f}s")           # :147
    finish(a, names, cls_ids, per_class, per_image_props, len(files))
    return 0


def run_seq(a, net, text, files, names, cls_ids, imgH, imgW, per_class):
    """--seq-nms: run_seq_clips with the plain stage's detect_merge_add; the result files as ever, --tubelets-out beside them."""
    from mscnn_amd import kitti

    def add(params, mviews, list_of):
        p = [dict(q, proposal_thr=a.proposal_thr, nms_overlap=a.nms_overlap) for q in params]
        net.detect_merge_add(p, cls_ids, views=mviews, list_of=list_of)

    frames, _, _ = run_seq_clips(a, net, text, files, (imgH, imgW), (1, 3, imgH, imgW), len(cls_ids), load_frame, add)
    a.track_ids = [t for _, _, t in frames]
    for k, (path, (dets, _, _)) in enumerate(zip(files, frames), start=1):
        by_type = {}
        for ci, c in enumerate(cls_ids):
            per_class[c].append(dets[ci])
            by_type[{"car": "Car", "ped": "Pedestrian", "cyc": "Cyclist"}.get(names[c - 1], names[c - 1])] = dets[ci]
        if a.labels_dir:
            kitti.write_kitti_labels(a.labels_dir, frame_id(path, k), by_type)
    finish(a, names, cls_ids, per_class, [], len(files))
    for ci, c in enumerate(cls_ids if a.tubelets_out else []):
        out = os.path.join(a.tubelets_out, f"{a.comp_id}_{names[c - 1]}.txt")
        write_tubelets(out, [d[ci] for d, _, _ in frames], [q[ci] for _, q, _ in frames])
        print(f"{out}: {len(set((k // a.clip, int(v)) for k, (_, q, _) in enumerate(frames) for v in q[ci]))} tubelets over {len(files)} images")
    return 0


def run_merged(a, net, text, files, names, cls_ids, imgH, imgW, per_class):
    """--scales / --flip: per frame one detect_merge_begin, per forward set_image + forward + detect_merge_add, one detect_merge_end."""
    import torch
    from mscnn_amd import kitti
    passes = merge_passes(a, (imgH, imgW))
    by_views = bool(a.tiles or a.views_batch)                                 # the views paths: set_image_views instead of a host mirror
    n_fwd = len(a.scales or [0]) * views_per_frame(a) if by_views else len(passes)
    cand_cap = merge_cand_cap(text, n_fwd, a.merge_cap)
    shape = (1, 3, imgH, imgW)
    used = 0.0
    apply_merge_settings(net, a)                                              # sticky: every detect_merge_end below votes / runs Soft-NMS

    def add(params, mviews, list_of):
        p = [dict(q, proposal_thr=a.proposal_thr, nms_overlap=a.nms_overlap) for q in params]
        net.detect_merge_add(p, cls_ids, views=mviews, **({} if list_of is None else dict(list_of=list_of)))

    for k, path in enumerate(files, start=1):
        img = load_frame(path, k)
        orgH, orgW = img.shape[:2]
        net.detect_merge_begin(1, len(cls_ids), cand_cap)
        if by_views:
            shape, dt = run_frame_views(a, net, img, a.scales or [(imgH, imgW)], shape, add)
            used += dt
        for H, W, flipped in () if by_views else passes:
            if (1, 3, H, W) != shape:
                shape = (1, 3, H, W)
                net.reshape_input("data", shape)
            frame = np.ascontiguousarray(img[:, ::-1]) if flipped else img
            dev_img = torch.from_numpy(frame).cuda(a.device)
            net.set_image("data", dev_img)
            torch.cuda.synchronize(a.device)
            t0 = time.perf_counter()
            net.forward()
            torch.cuda.synchronize(a.device)
            used += time.perf_counter() - t0                                  # forwards only, as :72-73
            p = dict(ratios=(H / float(orgH), W / float(orgW)), org_hw=(orgH, orgW), proposal_thr=a.proposal_thr, nms_overlap=a.nms_overlap)
            net.detect_merge_add([p], cls_ids, views=[dict(flip_x=1)] if flipped else None)
        set_group_streams(net, a, k - 1, 1)
        per_image, _ = net.detect_merge_end()
        a.track_ids += frame_tracks(net, a) or []
        render_frames(net, a, [img], [path], k)
        crop_frames(net, a, [img], [path], k)
        by_type = {}
        for ci, c in enumerate(cls_ids):
            dets = per_image[0][ci][0]
            per_class[c].append(dets)
            by_type[{"car": "Car", "ped": "Pedestrian", "cyc": "Cyclist"}.get(names[c - 1], names[c - 1])] = dets
        if a.labels_dir:
            kitti.write_kitti_labels(a.labels_dir, frame_id(path, k), by_type)
        if k % 100 == 0 or k == len(files):
            what = f"{n_fwd} views per frame, batched" if a.views_batch else f"{n_fwd} forwards per frame"
            print(f"idx {k}/{len(files)}, avgtime={used / k:.4f}s ({what})")
    finish(a, names, cls_ids, per_class, [], len(files))
    return 0


def run_batched(a, net, files, names, cls_ids, imgH, imgW, per_class, per_image_props, forward, rois=None):
    """--batch B: groups of B frames through set_images -> forward -> one detect_multi; results in frame order."""
    import torch
    from mscnn_amd import kitti
    used, n_in = 0.0, None
    for g0 in range(0, len(files), a.batch):
        group = files[g0:g0 + a.batch]
        if len(group) != n_in:                                                # the last group: the net at its own size
            net.reshape_input("data", (len(group), 3, imgH, imgW))
            n_in = len(group)
        dev_imgs = [torch.from_numpy(load_frame(path, g0 + i + 1)).cuda(a.device) for i, path in enumerate(group)]
        params = net.set_images("data", dev_imgs)                           # :63-69 for every frame of the group, on the device
        torch.cuda.synchronize(a.device)
        t0 = time.perf_counter()
        ran = True
        if rois is None:
            forward()
        elif sum(len(r) for r in rois[g0:g0 + len(group)]):
            net.forward_rois(group_rois(rois[g0:g0 + len(group)]), "image", params)
        else:
            ran = False                                                       # no frame of the group has a box
        torch.cuda.synchronize(a.device)
        used += time.perf_counter() - t0                                      # :72-73: forward only
        if a.proposals_out and not ran:
            per_image_props += [np.zeros((0, 5))] * len(group)
        elif a.proposals_out:                                                 # :75-91 for every frame of the group
            per_image_props += [pr for pr, _ in net.proposals_multi([dict(p, proposal_thr=a.proposal_thr) for p in params])[0]]
        if a.proposals_only:
            k = g0 + len(group)
            if k % 100 < len(group) or k == len(files):
                print(f"idx {k}/{len(files)}, avgtime={used / k:.4f}s")
            continue
        if ran:
            set_group_streams(net, a, g0, len(group))
            per_image, _ = net.detect_multi([dict(p, proposal_thr=a.proposal_thr, nms_overlap=a.nms_overlap) for p in params], cls_ids)
            a.track_ids += frame_tracks(net, a) or []
            render_frames(net, a, dev_imgs, group, g0 + 1)
            crop_frames(net, a, dev_imgs, group, g0 + 1)
        else:
            per_image = [[(np.zeros((0, 5)), None)] * len(cls_ids)] * len(group)
        for i, path in enumerate(group):
            k = g0 + i + 1
            by_type = {}
            for ci, c in enumerate(cls_ids):
                dets = per_image[i][ci][0]
                per_class[c].append(dets)
                by_type[{"car": "Car", "ped": "Pedestrian", "cyc": "Cyclist"}.get(names[c - 1], names[c - 1])] = dets
            if a.labels_dir:
                kitti.write_kitti_labels(a.labels_dir, frame_id(path, k), by_type)
            if k % 100 == 0 or k == len(files):
                print(f"idx {k}/{len(files)}, avgtime={used / (g0 + len(group)):.4f}s")   # per frame
    finish(a, names, cls_ids, per_class, per_image_props, len(files))
    return 0


def finish(a, names, cls_ids, per_class, per_image_props, n_files):
    if not a.proposals_only:
        write_results(a, names, cls_ids, per_class, n_files)
    if a.proposals_out:
        out = write_proposals(a.proposals_out, a.comp_id, per_image_props)
        print(f"{out}: {sum(len(p) for p in per_image_props)} proposals over {n_files} images")
    for ci, c in enumerate(cls_ids if track_on(a) and a.tracks_out else []):
        out = os.path.join(a.tracks_out, f"{a.comp_id}_{names[c - 1]}.txt")
        out = ", ".join(write_tracks(out, per_class[c], [t[ci] for t in a.track_ids], a.streams))
        print(f"{out}: {len(set(int(v) for t in a.track_ids for v in t[ci]) - {0})} tracks over {n_files} images")


def write_proposals(out_dir, comp_id, per_image_props):
    """dlmwrite(['proposals/' comp_id '.txt'], final_proposals) (:154, :161-162): rows [image_index x y w h score], %.5g."""
    from mscnn_amd import kitti
    out = os.path.join(out_dir, f"{comp_id}.txt")
    kitti.write_detections_dlm(out, per_image_props)
    return out


def write_results(a, names, cls_ids, per_class, n_files):
    from mscnn_amd import kitti
    for c in cls_ids:
        out = os.path.join(a.out, f"{a.comp_id}_{names[c - 1]}.txt")
        kitti.write_detections_dlm(out, per_class[c])                         # :150-161
        print(f"{out}: {sum(len(d) for d in per_class[c])} detections over {n_files} images")


if __name__ == "__main__":
    sys.exit(main())
