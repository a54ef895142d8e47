#!/usr/bin/env python3
"""The reference's second demo driver (examples/kitti_car/run_cascademscnn.m; the CityPersons and WiderFace copies differ in
constants) on the MI355X path: net from a deploy prototxt + weight file, every frame resized / BGR / mean-subtracted ON THE DEVICE
(:79-85), net.forward timed alone like the reference's tic / toc (:88-89), the post-processing loops over cascade outputs and
classes (:91-143) as ONE call per group of frames (Net.detect_cascade_multi), the result files
detections/<comp_id>_<class>_<output>_results.txt written as dlmwrite does (:148-158).

  python tools/run_cascademscnn.py --prototxt mscnn_deploy.prototxt --weights model.caffemodel --images /KITTI/testing/image_2
         [--outputs 1st,2nd,3rd] [--cls-ids 2] [--det-thr 0.05] [--nms-overlap 0.5] [--batch B] [--precision f32|f16x3|f16]
         [--out detections] [--comp-id cascade_mscnn] [--names bg,car,van,truck,tram] [--limit N]
         [--scales H1xW1,H2xW2,...] [--flip] [--merge-cap N]      # several forwards per frame, one NMS (Net.detect_merge_*)
         [--tiles RxC[:overlap_px]] [--views-batch]               # the frame cut into tiles; all views of a frame as ONE batched forward
         [--vote [THR]]                                           # box voting behind the merged NMS (Net.set_box_voting, THR default 0.5)
         [--soft-nms linear|gaussian[:SIGMA]] [--soft-thr T] [--max-dets N]      # Soft-NMS in place of the merged NMS (Net.set_soft_nms)
         [--matrix-nms linear|gaussian[:SIGMA]]              # Matrix NMS in its place instead (Net.set_matrix_nms); --soft-thr / --max-dets serve it
         [--wbf [THR]] [--wbf-skip T] [--wbf-conf avg|max] [--wbf-expected N]      # weighted boxes fusion in its place instead (Net.set_wbf)
         [--nms-type maxg|max] [--ovr-dnm union|min] [--nms-thr T]      # pNms.type / pNms.ovrDnm / bbNms's thr (Net.set_nms)
         [--roialign-one-pass]      # the ROIAlign heads of the net as one launch each (Net.set_roialign_one_pass; same results)
  python tools/run_cascademscnn.py --model kitti_car/cascade-mscnn-7s-576-2x --synthetic 8 --batch 2      # no dataset / weights at
                                                            # hand: the generated deploy net, seeded weights, synthetic frames
  python tools/run_cascademscnn.py --model widerface/cascade-mscnn-12s-align --images faces/ --orig-size [--max-size 3072]

--outputs: cascade outputs by the reference's names (1st, 2nd, 3rd, 3rd_avg), several at once if wanted.  Default: the last stage
as the reference picks it (:36-48) -- 3rd_avg when the net has cls_prob_3rd_avg, else 3rd, and 1st for a net without cascade stages.
--batch B runs B frames per forward (the net's input reshaped to (B, 3, H, W), the last group to its own size).
--orig-size is the WiderFace flow (widerface/run_cascademscnn.m:55, 82-91): every frame runs at its own size rounded to multiples
of 32 (scaled down to --max-size first when a side exceeds it), the net reshaped whenever that size changes; one frame per forward.
--scales / --flip run every frame at each of the given input sizes, with --flip a second time mirrored on the host ([:, ::-1]), and
merge the candidates of all those forwards before ONE NMS per cascade output and class (per frame Net.detect_merge_begin, per forward
Net.detect_cascade_merge_add, then Net.detect_merge_end; list size: forwards per frame x max_nms_num, or --merge-cap).  One frame per
forward, the same result files.  No reference script does this: there is no pin on the reference for it.  Without these flags the
driver runs exactly the calls it ran before they existed.
--tiles RxC[:overlap_px] cuts every frame into R x C equal, overlapping windows (mscnn_amd.net.tile_views) and runs each as a view,
resized on the device straight out of the uploaded frame (Net.set_image_views), with --flip each tile's mirror too; --views-batch
(with --flip and/or --tiles) runs all views of a frame in ONE forward: the input reshaped to N images, one set_image_views, one
forward, one detect_cascade_merge_add(..., list_of=), one detect_merge_end.  As tools/run_mscnn_detection.py; no pin on the reference.
--vote [THR] (default 0.5): every kept box becomes the score-weighted mean of all candidates of its output, class and frame whose IoU
with it is >= THR (Net.set_box_voting; on the device, between the merge and its read-back).  Alongside --scales / --flip / --tiles it
votes over their forwards; without them the frame runs as a merge of ONE forward.  As tools/run_mscnn_detection.py; no pin on the
reference, whose scripts neither merge nor vote.
--soft-nms linear|gaussian[:SIGMA] [--soft-thr T] [--max-dets N]: Soft-NMS in place of the merged hard NMS (Net.set_soft_nms; on the
device): overlapping candidates keep living with decayed scores.  As tools/run_mscnn_detection.py; alone a merge of ONE forward; no
pin on the reference, whose scripts neither merge nor decay a score.
--matrix-nms linear|gaussian[:SIGMA]: Matrix NMS in that place instead (Net.set_matrix_nms): every score decayed by its worst
compensated overlap with a higher-ranked candidate, no pick loop; --soft-thr / --max-dets serve it, not together with --soft-nms.  As
tools/run_mscnn_detection.py; alone a merge of ONE forward; not Soft-NMS's scores, no pin on the reference, accuracy not evaluated.
--wbf [THR] (default 0.55) [--wbf-skip T] [--wbf-conf avg|max] [--wbf-expected N]: weighted boxes fusion in that place instead
(Net.set_wbf): the candidates walked in score order into clusters, a cluster's box the score-weighted mean of its members, its
confidence scaled by min(members, N) / N; --max-dets serves it too; not together with --soft-nms, --matrix-nms or --vote.  As
tools/run_mscnn_detection.py; alone a merge of ONE forward; no pin on the reference, accuracy not evaluated.
--seq-nms [avg|max] [--clip T] [--seq-link THR] [--seq-top-k N] [--tubelets-out DIR]: Seq-NMS over clips of T frames (Net.set_seq_nms;
Han, Khorrami, Paine et al., 2016): one merge per clip with T lists per (output, class), every forward of --batch B frames added with
list_of naming its frames' places in the clip, the views of --flip / --scales / --tiles to their frame's list; --soft-thr, --max-dets
and --vote serve it; not together with --soft-nms, --matrix-nms or --wbf.  As tools/run_mscnn_detection.py; the result files keep their
format, --tubelets-out adds DIR/<comp_id>_<class>_<output>.txt with rows [image_index sequence x y w h score]; no pin on the reference,
accuracy not evaluated.
--track [--track-high T] [--track-low T] [--track-match THR] [--track-motion none|linear|kalman] [--track-max-age N] [--track-min-hits N]
[--track-kalman-pos S] [--track-kalman-vel S] [--track-kalman-keep-height 0|1] (with --track-motion kalman: a Kalman filter per track on
centre, aspect and height, Net.set_tracker_kalman; for jittering boxes, not for clean fast approaching ones, where linear overlaps better)
[--track-assign greedy|optimal] (the matching of both passes: the walk by descending IoU, the default, or the maximum-weight
assignment, Net.set_tracker_assign)
[--tracks-out DIR]: a persistent track id for every detection across the frames of the run, taken as consecutive frames of one stream
(Net.set_tracker; BYTE's two association passes on the device behind every detect_cascade_multi and detect_merge_end, a table of
tracks per (output, class)); alone, with --batch, with --orig-size (the boxes are original-image
pixels whatever the input size) and with every merge flag but --wbf.  As tools/run_mscnn_detection.py; the result files are unchanged, --tracks-out adds
DIR/<comp_id>_<class>_<output>.txt with rows [image_index track x y w h score], track 0 = no confirmed track (--streams N with
--track: the frames are N multiplexed cameras, frame i belongs to stream i % N and has that stream's tracks, --tracks-out writes
..._stream<s>.txt per stream; not with --seq-nms); no pin on the reference,
accuracy not evaluated.
--render-out DIR [--show-thr T] [--render-label none|score|id|both] [--render-color slot|id] [--pixelate N]: the `show` block of
run_cascademscnn.m:136-150 on the device (Net.render behind every detect_cascade_multi and detect_merge_end): DIR/<frame>.png with every
box of every (output, class) with a score >= T (default 0.3, the script's show_thr) outlined and labelled; --pixelate N replaces the
boxes' interiors with an N x N mosaic (anonymise the faces of a frame before it leaves the machine).  As tools/run_mscnn_detection.py;
the result files are unchanged; the look of the glyphs and colours is nobody's pin.
--crops-out DIR [--crop-size HxW] [--crop-thr T] [--crop-context F] [--crop-fit] [--crop-border clip|shift] [--crop-min N]
[--crop-tracked]: every detection of every (output, class) with a score >= T as a fixed-size patch, cut and resized on the device
(Net.crops behind every detect_cascade_multi and detect_merge_end, next to the render call): DIR/<frame>_<slot>_<row>.png, slot =
output x classes + class, with --track DIR/id<track>/<frame>_<slot>_<row>.png.  As tools/run_mscnn_detection.py; the result files are
unchanged.

Everything here is host glue over calls the test-suite covers one by one (Net.set_images, forward, detect_cascade_multi,
reshape_input, kitti.write_detections_dlm)."""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

OUTPUT_BLOBS = {   # the reference's output name -> (bbox blob, probability blob, proposal blob)
    "1st": ("output_bbox_1st", "cls_prob_1st", "proposals"),
    "2nd": ("output_bbox_2nd", "cls_prob_2nd", "proposals_2nd"),
    "3rd": ("output_bbox_3rd", "cls_prob_3rd", "proposals_3rd"),
    "3rd_avg": ("output_bbox_3rd", "cls_prob_3rd_avg", "proposals_3rd"),
}


def matlab_round(x):
    """MATLAB's round: halves away from zero (Python's round goes to the even neighbour: 22.5 -> 22)."""
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def net_input_size(org_h, org_w, max_size=3072):
    """The net input (H, W) of the --orig-size flow for a frame of org_h x org_w (widerface/run_cascademscnn.m:82-91): each side
    to the nearest multiple of 32; when either exceeds max_size, both scaled by max_size / the larger one and rounded again."""
    rz_h = matlab_round(org_h / 32.0) * 32
    rz_w = matlab_round(org_w / 32.0) * 32
    if rz_h > max_size or rz_w > max_size:
        t = max_size / float(max(rz_h, rz_w))
        rz_h = matlab_round(rz_h * t / 32.0) * 32
        rz_w = matlab_round(rz_w * t / 32.0) * 32
    return rz_h, rz_w


def default_outputs(blob_names):
    """The last stage as the reference picks it (:36-48)."""
    if "proposals_3rd" in blob_names:
        return ["3rd_avg" if "cls_prob_3rd_avg" in blob_names else "3rd"]
    return ["1st"]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--prototxt"); ap.add_argument("--weights", help=".caffemodel (new or V1 layout) or .h5 snapshot")
    ap.add_argument("--model", help="a deploy net of mscnn_amd.zoo instead of --prototxt (e.g. kitti_car/cascade-mscnn-7s-576-2x)")
    ap.add_argument("--input-size", default="", help="H,W: build the --model net at this input size instead of the deploy file's")
    ap.add_argument("--max-nms-num", type=int, default=0, help="BoxOutput's max_nms_num of the --model net (0: the deploy file's)")
    ap.add_argument("--images", help="directory of *.png / *.jpg frames")
    ap.add_argument("--synthetic", type=int, default=0, help="N synthetic frames instead of --images")
    ap.add_argument("--synthetic-sizes", default="375x1242", help="HxW[,HxW ...]: sizes of the synthetic frames, taken in turn")
    ap.add_argument("--outputs", default="", help="cascade outputs, comma separated: 1st, 2nd, 3rd, 3rd_avg (default: the last stage)")
    ap.add_argument("--out", default="detections"); ap.add_argument("--comp-id", default="cascade_mscnn_mi355x")
    ap.add_argument("--cls-ids", default="2", help="1-based class columns, comma separated (the reference's obj_ids)")
    ap.add_argument("--names", default="")
    ap.add_argument("--det-thr", type=float, default=0.0, help="> 0: drop detections under this probability before the NMS (:122-124)")
    ap.add_argument("--nms-overlap", type=float, default=0.5)
    ap.add_argument("--nms-type", default="maxg", choices=["maxg", "max"], help="pNms.type (bbNms.m: greedy or not)")
    ap.add_argument("--ovr-dnm", default="union", choices=["union", "min"], help="pNms.ovrDnm: the overlap's denominator")
    ap.add_argument("--nms-thr", type=float, default=None, help="bbNms's thr: drop rows with prob <= this before the NMS (default -inf)")
    ap.add_argument("--precision", default="f32", choices=["f32", "f16x3", "f16"])
    ap.add_argument("--limit", type=int, default=0); ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--batch", type=int, default=1, help="frames per forward")
    ap.add_argument("--orig-size", action="store_true", help="run every frame at its own size (multiples of 32), one frame per forward")
    ap.add_argument("--max-size", type=int, default=3072, help="--orig-size: scale frames down to this side length first")
    ap.add_argument("--dump-blobs", default="", help="directory: the cascade outputs' blobs and the frames' ratios / sizes of every "
                    "forward as group_NNNN.npz (to re-run the final stage on exactly what a forward produced)")
    ap.add_argument("--roialign-one-pass", action="store_true", help="run every ROIAlign head (two ROIAlign layers, their 2x2 AVE "
                    "poolings, the Concat: the WiderFace cascade's) as one launch (Net.set_roialign_one_pass); off: the five layers")
    from run_mscnn_detection import add_merge_flags, check_merge_flags, one_forward_merge, seq_on
    add_merge_flags(ap)
    a = ap.parse_args(argv)
    check_merge_flags(ap, a)
    if (a.scales or a.flip or a.tiles or one_forward_merge(a) or seq_on(a)) and (a.orig_size or a.dump_blobs):
        ap.error("--scales / --flip / --tiles / --vote / --soft-nms / --matrix-nms / --wbf name the input sizes themselves and keep no single forward's blobs: not with --orig-size / "
                 "--dump-blobs")
    if not (a.prototxt or a.model) or not (a.images or a.synthetic):
        ap.error("need --prototxt or --model, and --images or --synthetic N")
    if a.batch < 1:
        ap.error("--batch must be >= 1")
    if a.orig_size and a.batch > 1:
        ap.error(f"--orig-size with --batch {a.batch}: every frame runs at its own input size, and the images of one forward share "
                 "one; --orig-size runs one frame per forward (drop --batch)")
    for o in [o for o in a.outputs.split(",") if o]:
        if o not in OUTPUT_BLOBS:
            ap.error(f"--outputs {o}: not one of {', '.join(OUTPUT_BLOBS)}")
    if (a.input_size or a.max_nms_num) and not a.model:
        ap.error("--input-size / --max-nms-num change the generated --model net; a --prototxt is taken as it is")
    return a


def main(argv=None):
    a = parse_args(argv)
    import numpy as np
    import torch
    from mscnn_amd import kitti, net as mnet, synth, zoo
    from run_mscnn_detection import (apply_merge_settings, apply_track_setting, crop_frames, frame_tracks, list_images, load_rgb_u8, merge_cand_cap, merge_passes,
                                     names_for, one_forward_merge, render_frames, run_frame_views, run_seq_clips, seq_on, set_group_streams, track_on, views_per_frame,
                                     write_tracks, write_tubelets)

    if a.prototxt:
        text = open(a.prototxt).read()
    else:
        kw = {}
        if a.input_size:
            kw["height"], kw["width"] = (int(v) for v in a.input_size.split(","))
        if a.max_nms_num:
            kw["max_nms_num"] = a.max_nms_num
        text = zoo.prototxt(a.model, **kw)
    net = mnet.Net(prototxt_text=text, device=a.device)
    net.set_nms(type=a.nms_type, ovr_dnm=a.ovr_dnm, thr=a.nms_thr)      # sticky, like pNms at the top of the script
    if a.weights:
        net.load_caffemodel(a.weights)
    else:
        print("no --weights: seeded He-normal weights (synth.load_into) -- detections are meaningless, timings are not", file=sys.stderr)
        synth.load_into(net, "mid")
    if a.precision != "f32":
        net.set_precision(a.precision)
    if a.roialign_one_pass:
        net.set_roialign_one_pass(True)
    apply_track_setting(net, a)                                               # --track: sticky, every final stage below steps the tracks
    out_names = [o for o in a.outputs.split(",") if o] or default_outputs(net.blob_names)
    outputs = [OUTPUT_BLOBS[o] for o in out_names]
    for o, triple in zip(out_names, outputs):
        missing = [b for b in triple if b not in net.blob_names]
        if missing:
            sys.exit(f"--outputs {o}: the net has no blob {', '.join(missing)}")
    names = names_for(text, a.names)
    cls_ids = [int(c) for c in a.cls_ids.split(",")]
    files = list_images(a.images, a.limit) if a.images else [None] * a.synthetic
    if not files:
        sys.exit(f"no images in {a.images}")
    syn_sizes = [tuple(int(v) for v in s.split("x")) for s in a.synthetic_sizes.split(",")]

    def load_frame(path, k):      # frame k (1-based): the file, or a seeded uint8 RGB frame of the k-th synthetic size
        if path is not None:
            return load_rgb_u8(path)
        h, w = syn_sizes[(k - 1) % len(syn_sizes)]
        return np.ascontiguousarray(np.random.default_rng(1701 + k).integers(0, 256, (h, w, 3), dtype=np.uint8))

    shape = tuple(net.blob_shape("data"))
    results = {(o, c): [] for o in range(len(outputs)) for c in range(len(cls_ids))}
    used, done = 0.0, 0
    # --scales / --flip: several forwards per frame, one NMS per (output, class): one detect_merge_begin per frame, after every forward a
    # detect_cascade_merge_add (the mirrored forward with the view flip_x = 1), then one detect_merge_end
    # --tiles / --views-batch: the views come straight out of the frame uploaded once (Net.set_image_views), with --views-batch all of
    # them in ONE forward and one detect_cascade_merge_add(..., list_of=)
    # --vote: sticky box voting in every detect_merge_end; on its own the frame is a merge of one forward
    # --soft-nms: sticky Soft-NMS in place of that NMS; on its own a merge of one forward too
    # --seq-nms: the frames a clip at a time (run_seq_clips), every forward's rows to the lists of its frames' places in the clip
    passes = merge_passes(a, shape[2:]) if (a.scales or a.flip or a.tiles or one_forward_merge(a)) and not seq_on(a) else []
    if not seq_on(a):
        apply_merge_settings(net, a)
    by_views = bool(a.tiles or a.views_batch)
    n_fwd = len(a.scales or [0]) * views_per_frame(a) if by_views else len(passes)

    def add(params, mviews, list_of):
        net.detect_cascade_merge_add([dict(p, nms_overlap=a.nms_overlap) for p in params], outputs, cls_ids, det_thr=a.det_thr, views=mviews,
                                     **({} if list_of is None else dict(list_of=list_of)))

    tubes = {key: [] for key in results}
    tracks = {key: [] for key in results}                                     # --track: per frame the track ids of the key's detections
    if seq_on(a):
        frames, shape, used = run_seq_clips(a, net, text, files, tuple(shape[2:]), shape, len(outputs) * len(cls_ids), load_frame,
                                            lambda params, mviews, list_of: add(params, mviews, list_of))
        for dets, seqs, trks in frames:
            for (o, c) in results:
                results[(o, c)].append(dets[o * len(cls_ids) + c])
                tubes[(o, c)].append(seqs[o * len(cls_ids) + c])
                if trks is not None:
                    tracks[(o, c)].append(trks[o * len(cls_ids) + c])
    for k, path in enumerate(files if passes else [], start=1):
        img = load_frame(path, k)
        net.detect_merge_begin(1, len(outputs) * len(cls_ids), merge_cand_cap(text, n_fwd, a.merge_cap))
        if by_views:
            shape, dt = run_frame_views(a, net, img, a.scales or [tuple(shape[2:])], shape, add)
            used += dt
        for H, W, flipped in () if by_views else passes:
            if (1, 3, H, W) != shape:
                shape = (1, 3, H, W)
                net.reshape_input("data", shape)
            dev_imgs = [torch.from_numpy(np.ascontiguousarray(img[:, ::-1]) if flipped else img).cuda(a.device)]
            params = net.set_images("data", dev_imgs)
            torch.cuda.synchronize(a.device)
            t0 = time.perf_counter()
            net.forward()
            torch.cuda.synchronize(a.device)
            used += time.perf_counter() - t0
            net.detect_cascade_merge_add([dict(p, nms_overlap=a.nms_overlap) for p in params], outputs, cls_ids, det_thr=a.det_thr,
                                         views=[dict(flip_x=1)] if flipped else None)
        set_group_streams(net, a, k - 1, 1)
        per_image, _ = net.detect_merge_end()
        trks = frame_tracks(net, a)
        render_frames(net, a, [img], [path], k)
        crop_frames(net, a, [img], [path], k)
        for (o, c) in results:
            results[(o, c)].append(per_image[0][o * len(cls_ids) + c][0])
            if trks:
                tracks[(o, c)].append(trks[0][o * len(cls_ids) + c])
        if k % 100 == 0 or k == len(files):
            what = f"{n_fwd} views per frame, batched" if a.views_batch else f"{n_fwd} forwards per frame"
            print(f"idx {k}/{len(files)}, avgtime={used / k:.4f}s ({what})")
    for g0 in range(0, len(files) if not passes and not seq_on(a) else 0, a.batch):
        group = files[g0:g0 + a.batch]
        frames = [load_frame(path, g0 + i + 1) for i, path in enumerate(group)]
        H, W = net_input_size(frames[0].shape[0], frames[0].shape[1], a.max_size) if a.orig_size else shape[2:]
        if (len(group), 3, H, W) != shape:                                   # the last group, or --orig-size: another frame size
            shape = (len(group), 3, H, W)
            net.reshape_input("data", shape)
        dev_imgs = [torch.from_numpy(f).cuda(a.device) for f in frames]
        params = net.set_images("data", dev_imgs)                            # :77-85 for every frame of the group, on the device
        torch.cuda.synchronize(a.device)
        t0 = time.perf_counter()
        net.forward()
        torch.cuda.synchronize(a.device)
        used += time.perf_counter() - t0                                     # :88-89: forward only
        set_group_streams(net, a, g0, len(group))
        per_image, _ = net.detect_cascade_multi([dict(p, nms_overlap=a.nms_overlap) for p in params], outputs, cls_ids, det_thr=a.det_thr)
        if a.dump_blobs:
            os.makedirs(a.dump_blobs, exist_ok=True)
            blobs = {b: net.get_blob(b) for t in outputs for b in t}
            np.savez(os.path.join(a.dump_blobs, f"group_{g0 // a.batch:04d}.npz"), ratios=np.array([p["ratios"] for p in params], np.float64),
                     org_hw=np.array([p["org_hw"] for p in params], np.float64), **blobs)
        trks = frame_tracks(net, a)
        render_frames(net, a, dev_imgs, group, g0 + 1)
        crop_frames(net, a, dev_imgs, group, g0 + 1)
        for i in range(len(group)):
            for key in results:
                results[key].append(per_image[i][key[0]][key[1]][0])
                if trks:
                    tracks[key].append(trks[i][key[0] * len(cls_ids) + key[1]])
        done += len(group)
        if done // 100 != (done - len(group)) // 100 or done == len(files):
            print(f"idx {done}/{len(files)}, avgtime={used / done:.4f}s")    # :145, per frame
    for (o, c), dets in results.items():
        path = os.path.join(a.out, f"{a.comp_id}_{names[cls_ids[c] - 1]}_{out_names[o]}_results.txt")
        kitti.write_detections_dlm(path, dets)                               # :148-158
        print(f"{path}: {sum(len(d) for d in dets)} detections over {len(files)} images")
        if a.tubelets_out:
            write_tubelets(os.path.join(a.tubelets_out, f"{a.comp_id}_{names[cls_ids[c] - 1]}_{out_names[o]}.txt"), dets, tubes[(o, c)])
        if track_on(a) and a.tracks_out:
            out = os.path.join(a.tracks_out, f"{a.comp_id}_{names[cls_ids[c] - 1]}_{out_names[o]}.txt")
            out = ", ".join(write_tracks(out, dets, tracks[(o, c)], a.streams))
            print(f"{out}: {len(set(int(v) for t in tracks[(o, c)] for v in t) - {0})} tracks over {len(files)} images")
    return 0


if __name__ == "__main__":
    sys.exit(main())
