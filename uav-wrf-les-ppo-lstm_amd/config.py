# config.py -- hyper-parameters of the PPOV2.0/2.1 trainer.
#
# Same module-level names and values as the reference's PPOV2.0/config.py:6-44 and
# PPOV2.1/config.py:12-13, imported by name by environment.py / model.py / train_ppo2.0.py
# (drop-in surface).  The block at the end is additive: knobs of the MI355X build
# whose defaults reproduce the reference (one env, MLP policy, 256-step buffer).

GRID_SIZE = 500
MAX_STEPS = 1000
CONC_PEAK = 100.0
TURBULENCE_INTENSITY = 3.0

# Gaussian field of PPOV2.1 (PPOV2.1/config.py:12-13)
GAUSSIAN_RADIUS = 15.0
PEAK_CONCENTRATION = 100.0

# PPO
GAMMA = 0.99
LAMBDA = 0.95
CLIP_EPSILON = 0.2
ENTROPY_BETA = 0.01
LEARNING_RATE = 3e-5
BATCH_SIZE = 256
EPOCHS = 5

# exploration
EXPLORE_BONUS = 0.6
DECAY_FACTOR = 0.999
GRID_DIVISIONS = 10
EXPLORE_DECAY_ALPHA = 0.002

# curriculum
INITIAL_RADIUS = 50.0
MIN_RADIUS = 5.0
RADIUS_DECAY = 0.9
SUCCESS_THRESHOLD = 0.6
WINDOW_SIZE = 120

# reward shaping
CONC_REWARD_COEF = 2.0
TKE_PENALTY_FACTOR = 0.4
BOUNDARY_PENALTY = 0.1
BOUNDARY_DECAY_START = 0.15

TRAINING_SIZE = 10
SUCCESS_DISTANCE_THRESHOLD = 40
EVALUATE_SIZE = 10

# ---------------------------------------------------------------------------- MI355X build (additive)
ENV_VARIANT = "v2.0"     # "v2.0" sigma=500/16 | "v2.1" sigma=GAUSSIAN_RADIUS | "v1.1" clip 500-1e-6, MAX_STEPS 5000
DEVICE = "cuda"
NUM_ENVS = 1             # vectorised trainer: environments per GPU (BASELINE C3: 4096)
HORIZON = BATCH_SIZE     # rollout length per env (BASELINE C3: 128)
POLICY = "mlp"           # "mlp" = the reference's PPOActorCritic | "lstm" = LSTM actor-critic (BASELINE)
HIDDEN = 128             # LSTM hidden size (64 / 128)
NUM_LAYERS = 1
NUM_MINIBATCHES = 1      # the reference uses ONE minibatch of the whole buffer per epoch (train_ppo2.0.py:44-45)
SHUFFLE_ENVS = False     # True (with NUM_MINIBATCHES > 1): every epoch cuts a fresh permutation of the envs into the minibatches
BPTT_LEN = None          # LSTM: truncated BPTT over chunks of this many steps (divides HORIZON); None = whole env sequences
PPO_DIAGNOSTICS = False  # True: per-epoch approx. KL / clip fractions / explained variance of every update (update_diagnostics.csv)
TARGET_KL = None         # a positive number: stop an update's epochs once the epoch's approx. KL (k3) exceeds it; implies PPO_DIAGNOSTICS
NORMALISE_REWARDS = False  # True: the GAE reads the reward scaled by the running std of the discounted return (reward_norm_state.npz)
REWARD_CLIP = 10.0       # ... and clamped to +-REWARD_CLIP afterwards (None: no clamp)
NORMALISE_OBS = False    # True: running per-channel observation statistics folded into the policy's first layer (obs_norm_state.npz); the saved model is the folded one
OBS_NORM_EPS = 1e-4      # ... with inv_sigma = 1 / sqrt(var + OBS_NORM_EPS): at most 100, the bound of a channel that is constant so far
LR_SCHEDULE = "constant" # "linear": LEARNING_RATE -> LR_FINAL over SCHEDULE_ITERATIONS iterations | "adaptive": the rate follows the update's approx. KL (lr_state.npz)
LR_FINAL = None          # "linear": the rate from iteration SCHEDULE_ITERATIONS on
ENTROPY_BETA_FINAL = None  # a number: ENTROPY_BETA -> this over SCHEDULE_ITERATIONS iterations, under any LR_SCHEDULE; None keeps ENTROPY_BETA
SCHEDULE_ITERATIONS = None  # the iterations the two linear schedules run over (they hold their final value afterwards)
DESIRED_KL = None        # "adaptive": the rate is divided by LR_FACTOR after an update whose approx. KL (k3) exceeds 2 x this, multiplied below half of it; implies PPO_DIAGNOSTICS
LR_FACTOR = 1.5          # ... the factor of one such change
LR_MIN = 1e-6            # ... the lowest rate it reaches
LR_MAX = 1e-2            # ... and the highest; LEARNING_RATE starts inside [LR_MIN, LR_MAX]
EVAL_EVERY = None        # a number K: every K iterations one greedy episode on each of EVAL_ENVS fixed evaluation envs, on the device (eval_curve.csv, best_model.pth)
EVAL_ENVS = 256          # ... the evaluation envs per rank (their own env: the default radius, never touched by the curriculum)
EVAL_SEED = 4321         # ... and their seed; every evaluation runs the same episodes
EVAL_MAX_STEPS = None    # ... the step limit of an evaluation episode (None: the env's own)
EVAL_SOURCE_FIT = False  # ... also estimate the plume's source from each evaluation's records (True, or a dict of uavppo.source_fit.check_source_fit's keywords): six more columns in eval_curve.csv; {"model": "aniso"}: the six-term fit of stretched plumes (FIELD_BANK "aniso:F"), nine columns
EVAL_SOURCE_STOP = False  # ... and let that estimate stop the evaluation's episodes once it has settled (True, or a dict of uavppo.source_stop.check_source_stop's keywords; implies EVAL_SOURCE_FIT): a Stop_Rate column more.  The evaluation env's own success radius still ends episodes: give VecPPOTrainer a small eval_radius with it
KEEP_BEST = True         # ... keep the parameters of the best evaluation so far (most successes, then fewest steps) as best_model.pth
GAE_MODE = "reference_exact"   # or "standard" (PPOV1.0/ppo0.0.py:337-350)
SEED = 1234
BC_EPOCHS = 10           # behaviour cloning (train_bc.py): passes over the expert set ...
BC_BATCH = 4096          # ... in chunks of this many pairs (MLP) or whole episodes (LSTM), one optimiser step each
BC_LR = 3e-4             # its Adam step size
BC_VALUE_COEF = 0.0      # weight of the value regression, used only when value targets are given
TREND_K = 0              # extra observation channels obs[2](t) - obs[2](t-1-i), i < TREND_K (BASELINE C5: 2)
FIELD_BANK = None        # None = procedural fields | path to .npz / netCDF (conc, tke, source) | "synth:F" (BASELINE C4: "synth:64")
ITERATIONS = 200         # vectorised trainer: rollout + update iterations ...
EPISODES = None          # ... or stop once this many episodes have finished (the reference trains 2000, train_ppo2.0.py:128)
# data parallel, one process per GPU (torchrun / bench.py's launcher export these); 1 rank when absent
import os as _os
WORLD_SIZE = int(_os.environ.get("WORLD_SIZE", "1"))
RANK = int(_os.environ.get("RANK", "0"))
LOCAL_RANK = int(_os.environ.get("LOCAL_RANK", "0"))
DIST_BACKEND = _os.environ.get("UAVPPO_DIST_BACKEND", "nccl")   # "nccl" == RCCL over xGMI; "gloo" only for rehearsals / tests
