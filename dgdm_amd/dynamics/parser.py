"""Command-line flags shared by every entry point (reference: dynamics/parser.py:3-41).

Same flag names, types and defaults, so the shipped ``guided_sample_{2d,3d}.sh`` command lines parse unchanged."""
import argparse

# (flag, type | 'flag', default, help)
_FLAGS = [
    ("batch_size", int, 1024, "fingers per batch"),
    ("use_sub_batch", "flag", None, "split large classifier calls"),
    ("sub_bs", int, 1024, "rows per classifier call in 3-D guidance (fixes the FPS start partition)"),
    ("num_epochs", int, 1000, "training epochs (training is not part of this package)"),
    ("num_fingers", int, 1000, "size of the synthetic finger set"),
    ("ctrlpts_dim", int, 14, "control points per finger pair: 14 (2-D) or 42 (3-D)"),
    ("ctrlpts_x_dim", int, 7, "control net size along the finger"),
    ("ctrlpts_z_dim", int, 3, "control net size across the finger (3-D)"),
    ("learning_rate", float, 1e-4, "optimizer step size"),
    ("lr_warmup_steps", int, 100, "warm-up steps"),
    ("weight_decay", float, 0, "L2 penalty"),
    ("patience", int, 500, "early-stopping patience of dynamics training"),
    ("checkpoint_path", str, None, "dynamics model checkpoint (.pt, DataParallel state_dict)"),
    ("save_dir", str, None, "output directory"),
    ("wandb_id", str, None, "wandb run id"),
    ("data_dir", str, "", "training data"),
    ("test_data_dir", str, "", "held-out data"),
    ("object_dir", str, "", "objects: Icons-50 .npy (2-D) / scanned meshes (3-D) / objects.npy"),
    ("num_workers", int, 4, "DataLoader workers"),
    ("mode", str, "train", "'train' or 'test' (guided sampling)"),
    ("grid_size", int, 360, "orientations in the guidance grid"),
    ("num_pos", int, 9, "positions per axis in the guidance grid"),
    ("save_ckpt_step", int, 10, "checkpoint period"),
    ("val_step", int, 100, "validation period"),
    ("num_train_timesteps", int, 1000, "diffusion timesteps T"),
    ("num_timesteps_per_batch", int, 1, "timesteps drawn per training batch"),
    ("num_inference_steps", int, 100, "denoise steps S"),
    ("ema_power", float, 0.75, "EMA decay exponent"),
    ("object_max_num_vertices", int, 10, "points per object"),
    ("diffusion_checkpoint_path", str, None, "diffusion checkpoint (.ckpt, Lightning)"),
    ("classifier_guidance", "flag", None, "guide sampling with the dynamics model"),
    ("num_cpus", int, 4, "CPU workers of the (external) simulator"),
    ("fingers_3d", "flag", None, "3-D fingers / PointNet++ dynamics model"),
    ("render_video", "flag", None, "simulator videos (external)"),
    ("predicted_sim", "flag", None, "fill the objective tables with the dynamics model's predictions (dynamics/predicted.py)"),
    ("predicted_rollout", int, 0, "with --predicted_sim: interactions the dynamics model is iterated for per start orientation, so that the "
                                  "final_* scores and 'convergence' see a settled pose (40 = the simulator's count; 0 = one interaction)"),
    ("predicted_render", "flag", None, "with --predicted_sim, 3-D, objects from mesh files: also write <object>_<gripper>_gripper.png for every pair and, "
                                       "for settled poses asked with render_last, <object>_<gripper>/<v>.png (sim/render_mesh.py)"),
    ("squeeze_sim", "flag", None, "2-D, --mode=test: fill the objective tables with the squeeze simulator (sim/squeeze.py: a frictionless - with --squeeze_friction a jamming-by-friction -, "
                                  "quasi-static parallel-jaw squeeze; its own model, not MuJoCo's); the scores are marked 'simulated': 'squeeze'"),
    ("squeeze_sim_3d", "flag", None, "--fingers_3d, --mode=test, objects from mesh files: fill the objective tables with the sliced squeeze simulator "
                                     "(sim/squeeze.py SqueezeSimulator3D: the 2-D model on the finger grid's horizontal planes); marked "
                                     "'simulated': 'squeeze'"),
    ("squeeze_closing_steps", int, None, "with --squeeze_sim / --squeeze_sim_3d: grid steps the object climbs in one closing (default 6; untuned)"),
    ("squeeze_window", int, None, "with --squeeze_sim / --squeeze_sim_3d: half-width in cells of the neighbourhood a step searches (default 2; untuned)"),
    ("squeeze_friction", float, None, "with --squeeze_sim or --resample_potential squeeze (2-D only, refused with --squeeze_sim_3d): the Coulomb "
                                      "friction coefficient of the squeeze - poses whose two contacts hold the object are jammed and stay where "
                                      "they are (default: none, the frictionless model; untuned)"),
    ("squeeze_friction_3d", float, None, "with --squeeze_sim_3d: the Coulomb friction coefficient of the sliced squeeze, a 3-D antipodal jamming rule on "
                                         "the jaws' surface normals and the mesh triangles' normals (not --squeeze_friction's per-plane rule) - poses "
                                         "whose two contacts hold the object are jammed and stay where they are (default: none, the frictionless "
                                         "model; this project's own model, untuned, nothing claimed about MuJoCo)"),
    ("score_stats", str, None, "dynamics training: the stats.json sim/sim_2d.py or sim/sim_3d.py wrote beside its data; scores are divided by its score_std "
                               "instead of the reference's constants"),
    ("save_meshes", "flag", None, "also export every emitted gripper as OBJ meshes, collision pieces and gripper_<idx>.xml (assets/finger_mesh.py)"),
    ("save_objects", "flag", None, "2-D: also export the run's icon objects as meshes, convex pieces and object_<idx>.xml into every model root "
                                   "(assets/icon_process.py save_icon_objects)"),
    ("seed", int, 0, "seed of the start noise"),
    ("goal_pose", str, None, "THETA_DEG,X_CM,Y_CM: also guide and score designs toward this object pose (dgdm_amd/goal.py); the validation sweep "
                             "then adds guided/goal_... and multi/goal_... after the reference's objectives"),
    ("goal_weight", str, "1,0,0", "with --goal_pose: a,b,c weights of the rotation, x and y terms of the goal's pull"),
    ("goal_window_deg", float, 90.0, "with --goal_pose: half-width in degrees of the band of orientations pulled toward the goal (0 < w <= 180)"),
    ("goal_window_cm", float, 3.0, "with --goal_pose: half-width in centimetres of the band of positions pulled toward the goal"),
    ("goal_profile", str, "sign", "with --goal_pose: 'sign' (unit pull inside the window) or 'linear' (proportional, saturating at the window)"),
    ("goal_scale", float, None, "with --goal_pose: classifier scale of the goal chains (default: the scale of 'convergence'; untuned for goals)"),
    ("global_cond", str, None, "generator: FILE.npy of float32 condition rows [num_fingers][gc], row i for finger i of the dataset; the eps-net is then "
                               "built with global_cond_dim = gc and trained (--mode=train) or sampled (--mode=test) on (fingers, condition) pairs"),
    ("cfg_weight", float, 1.0, "with --global_cond: classifier-free guidance weight w of every sampling loop, eps = eps_u + w (eps_c - eps_u) with eps_u the "
                               "net on the all-zero condition row (1: the plain conditional eps, 0: the unconditional one)"),
    ("cond_drop_prob", float, 0.0, "with --global_cond, --mode=train: probability with which a training sample sees the all-zero condition row instead of "
                                   "its own (what classifier-free guidance needs the net to have learnt)"),
    ("label_out", str, None, "generator, --mode=label: FILE.npy the standardised condition rows of all --num_fingers dataset fingers are written to, "
                             "as --global_cond takes them; FILE_raw.npy (raw units) and FILE.json (the statistics, --cond_stats) go beside it "
                             "(dgdm_amd/label.py; needs --classifier_guidance: the labels are the dynamics model's predictions)"),
    ("label_layout", str, "mean", "with --mode=label: 'mean' (one block of columns, averaged over the objects) or 'per_object' (one block per object)"),
    ("label_rollout", int, 0, "with --mode=label: K > 0 adds the five settled columns of a predicted roll-out of K interactions"),
    ("label_source", str, "model", "with --mode=label: 'model' (the dynamics model's predictions; needs --classifier_guidance) or 'squeeze' (the squeeze "
                                   "simulator's closings, sim/squeeze.py: 2-D only, needs no dynamics model and no checkpoint; frictionless unless "
                                   "--squeeze_friction; honours --squeeze_closing_steps / --squeeze_window; its own model, not MuJoCo's) or 'squeeze_3d' "
                                   "(the sliced squeeze of --fingers_3d on <object_dir>/<name>/model.obj; frictionless only)"),
    ("label_settled", "flag", None, "with --label_source squeeze / squeeze_3d: add the five settled columns, from the start orientations run until they settle"),
    ("label_squeeze_cells", str, None, "with --label_source squeeze / squeeze_3d: the squeeze table's theta,x cells as T,X (default: the squeeze defaults)"),
    ("cond_stats", str, None, "generator, --mode=test: the FILE.json a labelling run wrote; with --cond_target the eps-net is built with its width"),
    ("cond_target", str, None, "with --cond_stats: NAME=VALUE,... in raw units (e.g. frac_clockwise=0.9,frac_up=0.7); every batch is sampled under "
                               "that condition row, columns not named at the dataset mean"),
    ("edit_from", str, None, "generator, --mode=test: FILE.npy of designs (n, L) or (n, L, 1) in sampler units, n >= batch_size (e.g. a vis_guided/<tag>/<obj>.npy "
                             "of an earlier run); batch b edits rows [b B, (b + 1) B): the guided chains of the sweep start from these designs instead of "
                             "from noise and are written under vis_edit/ (dgdm_amd/edit.py)"),
    ("edit_steps", int, None, "with --edit_from: how many of the schedule's last steps an edit runs, 1..num_inference_steps (default: all)"),
    ("pin", str, None, "with --edit_from: control points held at the design's value, indices and inclusive ranges like 0-6,10 (the first half of the "
                       "indices is the left finger)"),
    ("edit_band_mm", float, None, "with --edit_from: no control point moves further than this many millimetres from the design"),
    ("eta", float, 0.0, "generator, --mode=test: eta of the DDIM step in every sampling loop (0: the deterministic step, 1: the DDPM variance); the "
                        "noise is made on the device, keyed by (--noise_seed, chain, step) (dgdm_amd/scheduler.py; the classifier scales are untuned "
                        "for eta > 0)"),
    ("noise_seed", int, None, "with --eta: seed of the steps' noise (default: --seed)"),
    ("shared_step_noise", "flag", None, "with --eta: every chain of a launch draws the same step noise (common random numbers, for comparing "
                                        "objectives on equal noise)"),
    ("resample_every", int, None, "with --eta > 0 and --classifier_guidance: after every K-th DDIM step (never the last) the fingers of a chain are "
                                  "weighed by the dynamics model's objective at (x_t, t) and, where the weights have degenerated, promising fingers are "
                                  "copied over poor ones (dgdm_amd/resample.py; the mechanism is this project's own, no reference counterpart)"),
    ("resample_beta", float, None, "with --resample_every: inverse temperature of the weights, per grid cell of a finger (untuned; 0 never resamples)"),
    ("resample_ess", float, None, "with --resample_every: resample when the effective sample size falls below this fraction of the fingers "
                                  "(default 0.5; above 1: at every evaluation)"),
    ("resample_potential", str, "model", "with --resample_every: whose objective weighs the fingers - 'model' (the dynamics model's at (x_t, t)) or "
                                         "'squeeze' (the squeeze simulator's on the predicted clean design: 2-D only, frictionless unless --squeeze_friction is given, this project's "
                                         "own mechanism, not MuJoCo's; honours --squeeze_closing_steps / --squeeze_window) or 'squeeze_3d' (with --fingers_3d and objects from "
                                         "mesh files: the sliced squeeze of 3-D fingers, blind between two planes of the finger grid, frictionless; the same companions "
                                         "but --squeeze_friction)"),
    ("resample_squeeze_cells", str, None, "with --resample_potential squeeze / squeeze_3d: the squeeze table's theta,x cells as T,X (default: the squeeze defaults, "
                                          "720,241)"),
    ("device_dataset", "flag", None, "dynamics training: read every data file once, keep the dataset on the GPU and build each batch's rows there "
                                     "(dynamics/device_dataset.py); same batches, draws and results as the host loop"),
]


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser()
    for name, kind, default, helptext in _FLAGS:
        if kind == "flag":
            p.add_argument("--" + name, action="store_true", help=helptext)
        else:
            p.add_argument("--" + name, type=kind, default=default, help=helptext)
    return p


def parse(argv=None):
    return build_parser().parse_args(argv)
