"""RenderPeople scans end to end: the reference's `apps/rp_fitting.py` on the GPU.

`python -m bodyfitting_amd.renderpeople --target_dir ... --output_dir ...` takes a folder of textured scans (`<subject>/<name>.obj`, the
`*_30k.obj` decimations skipped) to fitted SMPL / SMPL-X (+D) parameters and textures with the reference's options, tasks and files
(DESIGN.md section 15):

- `render_data` renders the eight views of each scan (`texture_dropin.render_texture_mesh`, white background) and writes
  `images/%02d.png` (and `masks/%02d.png` with --use_mask), or reads them back when `images/00.png` exists and takes only the cameras
  (`pose_only=True`).
- the `openpose` task detects on the GPU with the GeneBody runner's code (`genebody.Detection`: `openpose.OpenPose`, and
  `openpose_hand.OpenPoseHand` for SMPL-X) in place of openpose.bin, with the reference's skip test, and writes the JSON files;
  `read_openpose` reads them back through `io.load_openpose`.
- the `smplify` task is `body_fitting.BodyFitting` with the scan (`use_mesh=True`, SMPL+D when `smpld` is a task); with --debug the
  runner then writes BodyFitting's fit-check overlays `smplify/smpl_fitting/%02d.png` on the GPU (`overlay.fit_overlays`).
- the `texfit` task is `texture_dropin.TextureFitting(smpl_uv_dir, render=True, debug=True)` on `smplify/{smpl_type}+d.obj`.
- the `output` task copies what BodyFitting wrote to `SMPL/<subject>.obj` and `SMPL/<subject>.npy`.

One OpenPose (and hand) estimator, one BodyFitting (its HMR network and one SMPLify per gender) and one TextureFitting live for the
whole run; PNG reads and writes go through a thread pool of `genebody.io_threads()`.

Deliberate deviations from the reference:
- the `output` task: the reference `cp`s debug/opt_smpl/{smpl_type}.obj and debug/{smpl_type}_paramters.npy, which BodyFitting never
  writes, and would put every subject's file under the same name; this copies smplify/{smpl_type}.obj and
  smplify/{smpl_type}_parameter.npy to SMPL/<subject>.obj / .npy, and a missing source is one stderr line;
- the overlays are written by the runner after BodyFitting returns (BodyFitting itself still writes none);
- OpenPose's --write_images skeleton renders and the face keypoints (`--face`) are not produced; with --debug one stderr line says so;
- TextureFitting's `video.mp4` files are not written (texture_dropin);
- `--openpose_dir` and `--smplx_with_smpl_init` are accepted and ignored, as the reference ignores the second.
"""
from __future__ import annotations

import argparse
import concurrent.futures
import csv
import functools
import os
import shutil
import sys

import numpy as np

from .genebody import Detection, io_threads, read_image, write_png

RENDER_SKIP = 12                  # BodyFitting.__call__'s render_skip default: the overlays are of use_frames[::12]


def config_parser():
    """rp_fitting.py:22-56, the same options and defaults; --device added"""
    parser = argparse.ArgumentParser(prog="python -m bodyfitting_amd.renderpeople")
    parser.add_argument("--target_dir", type=str, default="/data/ours_new", help='target directory storing obj data')
    parser.add_argument("--output_dir", type=str, default="./logs", help='output directory for fitted smpl and parameters')
    parser.add_argument("--openpose_dir", type=str, default="../openpose", help='directory of built openpose binary file (unused)')
    parser.add_argument("--info_dir", type=str, help='csv file which contains gender information')
    parser.add_argument('--debug', default=True, action='store_true', help='is output debug, false will speed up')
    parser.add_argument('--load_size', default=512, type=int, help='load size of image data')
    parser.add_argument('--tasks', nargs='+', type=str, default=['openpose', 'smplify', 'smpld', 'texfit', 'output'],
                        help='tasks to perform')
    parser.add_argument('--use_mask', default=False, action='store_true', help='smplify with human mask or not')
    parser.add_argument('--smpl_type', default="smpl", type=str, help='use smpl or smplx')
    parser.add_argument('--age', default="adult", type=str, help='use smpl/smplx or smil')
    parser.add_argument('--smplx_with_smpl_init', default=True, action='store_true',
                        help='if use smpl fitting result to initialize smplx fitting (unused)')
    parser.add_argument('--viewnum', type=int, default=8, help='use multiview data')
    parser.add_argument('--smpl_uv_dir', type=str, default="./data/smpl_uv", help='folder to smpl uv')
    parser.add_argument('--white_bkgd', default=True, action='store_true', help='white bkgd')
    parser.add_argument('--device', default=0, type=int, help='HIP device to run on')
    return parser


class runner(Detection):
    """rp_fitting.py:59-175 with the GPU stages.  The device objects can be injected: `render` (render_texture_mesh's signature),
    `bodyfitter` (BodyFitting's), `texturefitter` (TextureFitting's __call__) and `overlay` (overlay.fit_overlays'); by default they
    are the library's on --device.  `args.texfit_iters` / `args.texfit_size`, when set, are TextureFitting's iter_num /
    render_img_size (default 200 / 512, the reference's)."""

    def __init__(self, args, render=None, bodyfitter=None, texturefitter=None, overlay=None):
        self.options = args
        self.openpose_dir = args.openpose_dir
        self.use_mask = args.use_mask
        self.white_bkgd = args.white_bkgd
        self.smpl_type = args.smpl_type
        self.debug = args.debug
        self.viewnum = args.viewnum
        self.output_dir = args.output_dir
        self.use_hand_face = (self.smpl_type == 'smplx')
        self.load_size = args.load_size
        self.tasks = args.tasks
        self.device = int(getattr(args, "device", 0))
        self.subjects, self.meshfiles = self.get_subjects()
        if self.options.info_dir is not None and os.path.exists(self.options.info_dir):
            self.genders = []
            with open(self.options.info_dir, 'r') as info:
                reader = csv.reader(info)
                for row in reader:
                    self.genders.append('female' if int(row[1]) == 0 else 'male')
        else:
            self.genders = ['neutral' for _ in range(len(self.subjects))]
        if bodyfitter is None:
            from .body_fitting import BodyFitting
            bodyfitter = BodyFitting(self.options)
        self.bodyfitter = bodyfitter
        self.disp = 'smpld' in self.tasks
        if 'texfit' in self.tasks and texturefitter is None:
            from .texture_dropin import TextureFitting
            # rp_fitting.py:73 passes distutils' `debug` function: always true
            texturefitter = TextureFitting(args.smpl_uv_dir, render=True, debug=True, iter_num=int(getattr(args, "texfit_iters", 200)),
                                           render_img_size=int(getattr(args, "texfit_size", 512)), device=self.device)
        self.texturefitter = texturefitter
        if render is None:
            from .texture_dropin import render_texture_mesh
            render = functools.partial(render_texture_mesh, device=self.device)
        self.render = render
        if overlay is None:
            from .overlay import fit_overlays
            overlay = functools.partial(fit_overlays, device=self.device)
        self.overlay = overlay
        self._pool = None

    def get_subjects(self):
        subjects, meshes = [], []
        for path, subdirs, files in os.walk(self.options.target_dir):
            for name in files:
                if '.obj' in name:
                    if name[-8:] != "_30k.obj":
                        meshfile = os.path.join(path, name)
                        subject = meshfile.split('/')[-2]
                        subjects.append(subject)
                        meshes.append(meshfile)
        return subjects, meshes

    def _map(self, fn, items):
        if self._pool is None:
            self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=io_threads())
        return list(self._pool.map(fn, items))

    def render_data(self, subject, meshfile):
        imgdir = os.path.join(self.output_dir, subject, 'images')
        maskdir = os.path.join(self.output_dir, subject, 'masks')
        os.makedirs(imgdir, exist_ok=True)
        if self.use_mask:
            os.makedirs(maskdir, exist_ok=True)

        if os.path.exists(os.path.join(imgdir, '%02d.png' % 0)):          # the views of an earlier run
            paths = [os.path.join(imgdir, '%02d.png' % i) for i in range(self.viewnum)]
            if self.use_mask:
                paths += [os.path.join(maskdir, '%02d.png' % i) for i in range(self.viewnum)]
            decoded = self._map(read_image, paths)
            images, masks = decoded[:self.viewnum], decoded[self.viewnum:]
            glRts, Ks = self.render(meshfile, self.load_size, pose_only=True)
        else:
            images, masks, glRts, Ks = self.render(meshfile, self.load_size, white_bkgd=self.white_bkgd)
            jobs = [(os.path.join(imgdir, '%02d.png' % i), images[i]) for i in range(self.viewnum)]
            if self.use_mask:
                jobs += [(os.path.join(maskdir, '%02d.png' % i), masks[i]) for i in range(self.viewnum)]
            self._map(lambda a: write_png(*a), jobs)
        Rts = [np.linalg.inv(Rt).astype(np.float32) for Rt in glRts]   # cv w2c
        Ks = [K.astype(np.float32) for K in Ks]
        use_frames = list(range(self.viewnum))
        mask_frames = list(range(self.viewnum))
        return images, masks, Ks, Rts, use_frames, mask_frames

    def run_openpose(self, subject, data):
        """openpose.bin --image_dir images --write_json openpose [--hand] (:118-128) on the GPU, with the reference's skip test"""
        wrt_dir = os.path.abspath(os.path.join(self.output_dir, subject, 'openpose'))
        os.makedirs(wrt_dir, exist_ok=True)
        if len([dir_ for dir_ in os.listdir(wrt_dir) if '.json' in dir_]) >= len(data[0]):
            return
        self.detect_and_write(data[0], data[4], wrt_dir)

    def read_openpose(self, subject):
        from .io import load_openpose
        openpose_dir = os.path.join(self.output_dir, subject, 'openpose')
        views = sorted([dir_ for dir_ in os.listdir(openpose_dir) if '.json' in dir_])
        return [load_openpose(os.path.join(openpose_dir, view)) for view in views]

    def run_smplify(self, subject, data, keypoints, gender, meshfile):
        images, masks, Ks, Rts, use_frames, mask_frames = data
        keyframe = use_frames[0]
        output_dir = os.path.join(self.output_dir, subject, 'smplify')
        result = self.bodyfitter(images, Rts, Ks, keypoints, gender=gender, keyframe=keyframe, use_frames=use_frames,
                                 use_mask=self.use_mask, masks=masks, mask_frames=mask_frames, output_folder=output_dir,
                                 use_mesh=True, meshfile=meshfile, disp=self.disp)
        if self.debug:                       # body_fitting.py:100-107, which BodyFitting here leaves to its caller
            self.write_overlays(output_dir, data, result)
        return result

    def write_overlays(self, output_dir, data, result):
        images, _, Ks, Rts, use_frames, _ = data
        fitting_path = os.path.join(output_dir, "smpl_fitting")
        os.makedirs(fitting_path, exist_ok=True)
        frames = use_frames[::RENDER_SKIP]
        outs = self.overlay(images, result["vertices"], Rts, Ks, frames, use_frames)
        self._map(lambda a: write_png(*a), [(os.path.join(fitting_path, '%02d.png' % f), o) for f, o in zip(frames, outs)])

    def run_texfit(self, subject, meshfile):
        output_dir = os.path.join(self.output_dir, subject, 'texfit')
        smpld_dir = os.path.join(self.output_dir, subject, 'smplify', f'{self.smpl_type}+d.obj')
        if os.path.exists(smpld_dir):
            self.texturefitter(output_dir, smpld_dir, meshfile)

    def run_output(self, subject):
        """:162-169 copies debug/ files BodyFitting never writes; this copies what it did write"""
        frame_dir = os.path.join(self.output_dir, subject)
        smpl_folder = os.path.join(self.output_dir, 'SMPL')
        os.makedirs(smpl_folder, exist_ok=True)
        for src, dst in ((os.path.join(frame_dir, 'smplify', f'{self.smpl_type}.obj'), os.path.join(smpl_folder, f'{subject}.obj')),
                         (os.path.join(frame_dir, 'smplify', f'{self.smpl_type}_parameter.npy'), os.path.join(smpl_folder, f'{subject}.npy'))):
            if os.path.exists(src):
                shutil.copyfile(src, dst)
            else:
                print(f"bodyfitting_amd.renderpeople: {src} does not exist, not copied", file=sys.stderr)

    def run(self):
        if self.debug:
            print("bodyfitting_amd.renderpeople: --debug outputs of OpenPose (skeleton images, face keypoints) are not produced",
                  file=sys.stderr)
        for subject, meshfile, gender in zip(self.subjects, self.meshfiles, self.genders):
            data = self.render_data(subject, meshfile)
            if 'openpose' in self.tasks:
                self.run_openpose(subject, data)
            keypoints = self.read_openpose(subject)
            if 'smplify' in self.tasks:
                self.run_smplify(subject, data, keypoints, gender, meshfile)
            if 'texfit' in self.tasks:
                self.run_texfit(subject, meshfile)
            if 'output' in self.tasks:
                self.run_output(subject)

    def close(self):
        bf = self.bodyfitter
        objs = [self._openpose, self._openpose_hand, getattr(self.texturefitter, "inpainter", None)]
        objs += [getattr(bf, "_hmr", None), getattr(bf, "_openpose", None), getattr(bf, "_openpose_hand", None)]
        objs += list(getattr(bf, "_fitters", {}).values())
        for obj in objs:
            if obj is not None and hasattr(obj, "close"):
                obj.close()
        self._openpose = self._openpose_hand = None
        for name in ("_hmr", "_openpose", "_openpose_hand"):     # BodyFitting makes them again if it is called after this
            if getattr(bf, name, None) is not None:
                setattr(bf, name, None)
        if getattr(bf, "_fitters", None):
            bf._fitters.clear()
        if getattr(self.texturefitter, "inpainter", None) is not None:
            self.texturefitter.inpainter = None
        if self._pool is not None:
            self._pool.shutdown()
            self._pool = None


def main(argv=None):
    args = config_parser().parse_args(argv)
    r = runner(args)
    try:
        r.run()
    finally:
        r.close()


if __name__ == "__main__":
    main()
