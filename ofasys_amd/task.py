"""`Task`: one instruction + its datasets + preprocessing + criterion settings (reference: task/base.py:157-460, 586-615,
839-865; exported as `ofasys.Task`, ofasys/__init__.py:65).

    task = Task(name="caption", instruction="[IMAGE:image] what does the image describe? -> [TEXT:caption]", micro_batch_size=4)
    task.add_dataset(rows, "train")            # any sequence of dict rows: datasets.Dataset, list of dicts, ...

Generation: `Task.generator` / `Task.inference` run beam search (ofasys_amd/generator.py SequenceGenerator; task/base.py:232-246,
470-556, 727-793) for TEXT targets and the autoregressive speech generator (AutoRegressiveSpeechGenerator; task/base.py:555-561) for
AUDIO targets.
Validation: `Task.valid_batches` walks a split once, in order; `Trainer.validate` (engine.py) runs it through the step engine's
forward-only `valid_step` -- loss, NLL and, with `cfg.criterion.report_accuracy`, token accuracy (task/base.py:680-703).
What stays out: file / OSS readers, multi-worker prefetch, generation metrics, the image / motion generators and the vocoder, checkpoint state.  The
batch iterator is a plain in-process loop over the bound dataset: micro-batches of `micro_batch_size` rows, each rank of a
data-parallel job reading its own contiguous shard (io/reader/dataset.py:49-53), reshuffled per epoch with a seeded permutation.
"""
import json
import random
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Set, Union

import numpy as np
import torch

from .preprocessor.collate import (BoxPreprocessConfig, DefaultBoxPreprocess, DefaultTextPreprocess, GeneralPreprocess,
                                   PreprocessConfig, TensorPreprocess, TextPreprocessConfig, default_preprocess)
from .preprocessor.audio import FbankPreprocess
from .preprocessor.motion import Motion6dPreprocess
from .preprocessor.instruction import Instruction, ModalityType, Slot

# adaptor/general.py:36-46
default_adaptor = {
    ModalityType.TEXT: "text", ModalityType.IMAGE: "image_resnet", ModalityType.BOX: "text", ModalityType.AUDIO: "audio_fbank",
    ModalityType.PHONE: "text", ModalityType.VIDEO: "video_image_sequence", ModalityType.MOTION: "text",
    ModalityType.STRUCT: "text", ModalityType.CATEGORY: "text",
}


@dataclass
class DatasetConfig:                                  # task/base.py:48-120 (fields the in-process iterator uses)
    micro_batch_size: int = 1
    update_freq: int = 1
    shuffle: bool = True
    seed: int = 1


@dataclass
class InstructionConfig:                              # task/base.py:123-137
    template: Optional[str] = None
    decoder_plain_with_loss: bool = False


@dataclass
class CriterionConfig:                                # engine/criterion/label_smoothed_cross_entropy.py:27-59 / cross_entropy.py
    label_smoothing: float = 0.0
    drop_worst_ratio: float = 0.0
    report_accuracy: bool = False                     # validation also reports n_correct / total / accuracy (:49-52, :180-198)
    # "scst_reward_criterion" (engine/criterion/scst_loss.py:39-56; used by a task with cfg.scst): the fields below are its own
    # "speech_to_text_loss" (engine/criterion/speech_to_text_loss.py:24-95): ce_weight * the label-smoothed loss on the decoder +
    # ctc_weight * CTC on the encoder output projected onto the '<phone>_dict_begin' .. '<phone>_dict_end' rows of the token embedding
    # (cfg.text.phone_dict registers them); ce_weight, ctc_weight, zero_infinity (and sentence_avg) are its own, the reference's defaults
    # "ofa_tacotron2" (engine/criterion/tacotron2_loss.py:24-45; a task whose target slot is [AUDIO:fbank]): bce_pos_weight and
    # sentence_avg are honoured; use_guided_attention_loss = True and its own ctc_weight > 0 are refused before the model runs
    # "diffusion_criterion" (engine/criterion/diffusion_loss.py:15-31; a task whose target slot is [MOTION:...,adaptor=motion_6d], with
    # TaskConfig.diffuser_args): scale_main_loss and weight scale the loss; scale_aux_loss_1 / scale_aux_loss_2 > 0 are refused before
    # the model runs (custom_reg_loss needs the BVH forward kinematics)
    name: str = "label_smoothed_cross_entropy"
    weight: float = 1.0
    scale_main_loss: float = 1.0
    scale_aux_loss_1: float = 0.0
    scale_aux_loss_2: float = 0.0
    bce_pos_weight: float = 1.0
    use_guided_attention_loss: bool = False
    ce_weight: float = 1.0
    ctc_weight: float = 0.0
    zero_infinity: bool = False
    scst_cider_cached_tokens: Any = "corpus"          # a pickle path (ref_len, document_frequency), such a dict, or "corpus"
    sentence_avg: bool = False
    ignore_prefix_size: int = 0
    constraint_range: Optional[str] = None


@dataclass
class EvaluationConfig:                               # task/base.py:138-153 (the generator arguments; metrics stay out)
    generator_args: str = '{"beam":5,"max_len_b":32,"no_repeat_ngram_size":3}'


@dataclass
class ImagePreprocessConfig(PreprocessConfig):        # preprocessor/default/image.py (resize + mean/std 0.5 normalisation)
    patch_image_size: int = 224
    mean: float = 0.5
    std: float = 0.5


@dataclass
class TaskConfig:                                     # task/base.py:157-189
    dataset: DatasetConfig = field(default_factory=DatasetConfig)
    instruction: InstructionConfig = field(default_factory=InstructionConfig)
    criterion: CriterionConfig = field(default_factory=CriterionConfig)
    evaluation: EvaluationConfig = field(default_factory=EvaluationConfig)
    text: TextPreprocessConfig = field(default_factory=TextPreprocessConfig)
    box: BoxPreprocessConfig = field(default_factory=BoxPreprocessConfig)
    image: ImagePreprocessConfig = field(default_factory=ImagePreprocessConfig)
    max_src_length: int = 128
    max_tgt_length: int = 30
    constraint_range: Optional[str] = None
    scst: bool = False                                # self-critical sequence training (task/base.py:170-174)
    scst_args: str = "{}"                             # generation arguments of the SCST generator, as JSON
    # the noise schedule of diffusion training, as JSON (task/base.py:176-179; diffusion.NoiseSchedule lists the keys)
    diffuser_args: str = '{"scheduler": "DDIMScheduler", "num_inference_steps": 50}'
    _name: Optional[str] = None

    def update(self, **kwargs):
        if "name" in kwargs:
            self._name = kwargs["name"]
        if "instruction" in kwargs:
            self.instruction.template = kwargs["instruction"]
        if "micro_batch_size" in kwargs:
            self.dataset.micro_batch_size = kwargs["micro_batch_size"]


def parse_template(template: Union[None, str, List[str]]) -> Optional[List[str]]:
    """A task may carry several alternative templates: a list, or one string with '||' between them."""
    if template is None:
        return None
    if isinstance(template, str):
        return [t.strip() for t in template.split("||") if t.strip()]
    return list(template)


class ImageTensorPreprocess(TensorPreprocess):
    """IMAGE / VIDEO columns that are already arrays: CHW float tensors pass through; HWC uint8 arrays (or PIL images) are
    scaled to [0,1], resized (bilinear) to patch_image_size and normalised with mean = std = 0.5.  File / URL decoding is out
    of scope."""

    def map(self, slot: Slot) -> Slot:
        v = slot.value
        if hasattr(v, "convert") and not torch.is_tensor(v):          # PIL.Image
            v = np.asarray(v.convert("RGB"))
        if isinstance(v, np.ndarray):
            v = torch.from_numpy(v)
        if not torch.is_tensor(v):
            raise ValueError(f"image slot '{slot.column_name}': expected a tensor / array / PIL image, got {type(v)} "
                             "(decoding files or URLs is outside this package)")
        if v.dtype == torch.uint8:
            if v.dim() == 3 and v.shape[-1] in (1, 3):
                v = v.permute(2, 0, 1)
            v = v.float() / 255.0
            size = self.cfg.patch_image_size
            if v.shape[-2:] != (size, size):
                v = torch.nn.functional.interpolate(v[None], size=(size, size), mode="bilinear", align_corners=False)[0]
            v = (v - self.cfg.mean) / self.cfg.std
        slot.value = v.float()
        return slot


class Task:
    def __init__(self, cfg: TaskConfig = None, **kwargs):
        self.cfg = TaskConfig() if cfg is None else cfg
        self.cfg.update(**kwargs)
        self.datasets: Dict[str, Any] = {}
        self.templates = parse_template(self.cfg.instruction.template)
        self.target_modality = self.infer_target_modality(self.templates[0]) if self.templates else None
        self.global_dict = None
        self.general_preprocess: Optional[GeneralPreprocess] = None
        self._iters = {}
        self._generator = None
        self._scst_generator = None
        self._sampling_gens: Dict[Any, Any] = {}
        self._diverse_gens: Dict[Any, Any] = {}
        self._trie_dev: Dict[Any, Any] = {}                  # device -> (plan, its device arrays): constraint_trie_on
        from .diffusion import parse_diffuser_args
        self.diffuser_args = parse_diffuser_args(self.cfg.diffuser_args)       # (task/base.py:207; an unknown key or value raises here)
        self._noise_schedule = None
        if self.cfg.criterion.name == "diffusion_criterion":
            self._check_diffusion_target()

    # ------------------------------------------------------------------ identity / datasets (task/base.py:256-273)
    @property
    def name(self):
        return self.cfg._name or self.__class__.__name__

    def add_dataset(self, dataset, split="train"):
        assert self.datasets.get(split) is None, f"{split} dataset already exists in task {self.name}"
        self.datasets[split] = dataset

    def add_train_dataset(self, dataset):
        self.add_dataset(dataset, "train")

    def add_valid_dataset(self, dataset):
        self.add_dataset(dataset, "valid")

    def add_test_dataset(self, dataset):
        self.add_dataset(dataset, "test")

    def _check_diffusion_target(self):
        """diffusion_criterion trains continuous motion frames only: every template's target slot must be MOTION with adaptor=motion_6d."""
        for template in self.templates or []:
            slot = Slot.get_target_slot_from_slots(Instruction(template).slots)
            if slot.modality != ModalityType.MOTION or slot.get_attr("adaptor") != "motion_6d":
                raise ValueError(f"task {self.name}: criterion diffusion_criterion needs a [MOTION:...,adaptor=motion_6d] target slot, "
                                 f"got [{slot.modality.name}] with adaptor={slot.get_attr('adaptor')!r}")

    @property
    def noise_schedule(self):
        """diffusion.NoiseSchedule(**diffuser_args), built once: the step engine's captured graphs address its device tables."""
        if self._noise_schedule is None:
            from .diffusion import NoiseSchedule
            self._noise_schedule = NoiseSchedule(**self.diffuser_args)
        return self._noise_schedule

    def infer_target_modality(self, instruction: Union[str, Instruction]):
        if not isinstance(instruction, Instruction):
            instruction = Instruction(instruction)
        return Slot.get_target_slot_from_slots(instruction.slots).modality

    # ------------------------------------------------------------------ set-up (task/base.py:218-231, 328-338)
    def initialize(self, global_dict, **kwargs):
        """Registers this task's symbols in the shared dictionary ('<text>_i', '<mask>', '<bin>_k') and builds its preprocessors."""
        self.global_dict = global_dict
        if "<text>_0" not in global_dict:
            from .preprocessor.tokenizer import N_GPT2
            for i in range(N_GPT2):
                global_dict.add_symbol(f"<text>_{i}")
        global_dict.add_symbol("<mask>")
        self.cfg.text.max_src_length, self.cfg.text.max_tgt_length = self.cfg.max_src_length, self.cfg.max_tgt_length
        name2pre = {"text": DefaultTextPreprocess(global_dict, self.cfg.text), "box": DefaultBoxPreprocess(global_dict, self.cfg.box)}
        for name, mod in (("image", ModalityType.IMAGE), ("video", ModalityType.VIDEO)):
            name2pre[name] = ImageTensorPreprocess(global_dict, self.cfg.image, mod)
        # (source-side and plain tensor values as TensorPreprocess; a target-side fbank slot collates as a text-to-speech target)
        name2pre["audio"] = FbankPreprocess(global_dict, PreprocessConfig(), ModalityType.AUDIO)
        name2pre["table"] = name2pre["phone"] = name2pre["text"]     # STRUCT / PHONE columns arrive as token ids (text adaptor)
        name2pre["motion_6d"] = Motion6dPreprocess(global_dict)      # rot6d frames: a slot selects it with preprocess=motion_6d
        self.general_preprocess = GeneralPreprocess(global_dict, name2pre)

    @classmethod
    def upgrade_model_adaptor_cfg(cls, tasks, model_cfg):
        """Activate exactly the adaptors the tasks' instructions need (task/base.py:228-231, 839-865)."""
        for name in collect_adaptor_name_from_tasks(tasks):
            getattr(model_cfg.adaptor, name).is_active = True

    # ------------------------------------------------------------------ rows -> samples (task/base.py:291-326, 389-394)
    def preprocess(self, data: Dict[str, Any], split: str) -> Dict[str, Any]:
        return data

    def build_instruction(self, data: Dict[str, Any], split: str) -> Instruction:
        template = random.choice(self.templates) if len(self.templates) > 1 else self.templates[0]
        return Instruction(template, split=split, decoder_plain_with_loss=self.cfg.instruction.decoder_plain_with_loss).format(**data)

    def preprocess_data_and_instruction(self, data, split):
        data = self.preprocess(data, split)
        if data is None:
            return None
        return self.general_preprocess(self.build_instruction(data, split))

    def collate(self, rows: List[Dict[str, Any]], split="train") -> Dict:
        samples = [s for s in (self.preprocess_data_and_instruction(dict(r), split) for r in rows) if s is not None]
        return self.general_preprocess.collate(samples)

    def constraint_trie_on(self, device):
        """The answer trie of the text preprocessor's closed set as the device arrays the node-form criterion reads
        (ops.trie_label_smoothed_cross_entropy): {"node_edge_off" int32 [N + 1], "edge_token" int32 [E], "N", "E"}.  Built once per
        device and handed out as the SAME tensors every time, so a captured step's replay finds nothing to copy.  Needs
        cfg.text.closed_set_nodes and a prepared closed set (the preprocessor's `constraint_plan`)."""
        plan = self.general_preprocess.name2pre["text"].constraint_plan if self.general_preprocess is not None else None
        if plan is None:
            raise ValueError(f"task {self.name}: no answer trie -- set cfg.text.closed_set_nodes and prepare a closed set")
        cache, key = self._trie_dev, torch.device(device)
        if key not in cache or cache[key][0] is not plan:      # (a closed set prepared again: a new plan, new arrays)
            # (with the inverse CSR by token, edge_node, node_ids, U and max_degree: what the trie-edge head reads as well)
            cache[key] = (plan, plan.head_arrays(key))
        return cache[key][1]

    # ------------------------------------------------------------------ iteration (task/base.py:396-449, in process)
    def _batches(self, split, rank, world):
        ds = self.datasets[split]
        n = len(ds)
        per = n // world if n >= world else n                       # contiguous per-rank shard (io/reader/dataset.py:49-53)
        lo = (rank * per) % max(n, 1)
        bs = self.cfg.dataset.micro_batch_size
        epoch = 0
        while True:
            order = list(range(lo, lo + per))
            if split == "train" and self.cfg.dataset.shuffle:
                np.random.default_rng(self.cfg.dataset.seed + epoch).shuffle(order)
            for i in range(0, len(order) - bs + 1 if len(order) >= bs else 1, bs):
                idx = order[i:i + bs]
                yield self.collate([ds[int(j) % n] for j in idx], split)
            epoch += 1

    def valid_batches(self, split="valid", rank=0, world=1):
        """A FINITE iterator over the rank's shard of `split` for one validation pass (task/base.py:680-703 with the reference's
        non-shuffled eval iterator): every row once, in dataset order, micro_batch_size rows per batch and the last, shorter batch
        included.  The shards are contiguous and together cover the whole dataset: rank r reads rows [r n / world, (r + 1) n / world)."""
        ds = self.datasets[split]
        n = len(ds)
        lo, hi = rank * n // world, (rank + 1) * n // world
        bs = self.cfg.dataset.micro_batch_size
        for i in range(lo, hi, bs):
            yield self.collate([ds[int(j)] for j in range(i, min(i + bs, hi))], split)

    def init_data_iterator(self, split="train", rank=0, world=1):
        self._iters[split] = self._batches(split, rank, world)

    def get_sample(self, split="train"):
        if split not in self._iters:
            self.init_data_iterator(split)
        return next(self._iters[split])

    # ------------------------------------------------------------------ generation (task/base.py:232-246, 470-556, 727-793)
    def generator_kwargs(self, **gen_kwargs) -> Dict[str, Any]:
        """The reference's generator arguments (task/base.py:475-486: its pops and defaults; normalize_scores defaults to False
        here, unlike the generator's own default) as SequenceGenerator keywords.  Beam search only: diverse beam, diverse siblings,
        match_source_len and lexical constraints raise NotImplementedError, and so do the sampling arguments -- a sampling
        generator comes from `sampling_generator`, a diverse one from `diverse_generator`."""
        args = dict(
            beam_size=gen_kwargs.pop("beam", 5), return_n_best=gen_kwargs.pop("return_n_best", 1),
            max_len_a=gen_kwargs.pop("max_len_a", 0), max_len_b=gen_kwargs.pop("max_len_b", 200),
            max_len=gen_kwargs.pop("max_len", 256), min_len=gen_kwargs.pop("min_len", 1),
            normalize_scores=gen_kwargs.pop("normalize_scores", False), len_penalty=gen_kwargs.pop("lenpen", 1),
            unk_penalty=gen_kwargs.pop("unkpen", 0), temperature=gen_kwargs.pop("temperature", 1.0),
            no_repeat_ngram_size=gen_kwargs.pop("no_repeat_ngram_size", 0))
        unsupported = {"sampling": False, "sampling_topk": -1, "sampling_topp": -1.0, "diverse_beam_groups": -1,
                       "diversity_rate": -1, "match_source_len": False, "constrained": False, "constraints": None}
        for k, default in unsupported.items():
            v = gen_kwargs.pop(k, default)
            if v != default:
                hint = "; for sampling call Task.sampling_generator(...)" if k.startswith("sampling") else \
                    "; for diverse decoding call Task.diverse_generator(...)" if k.startswith("divers") else ""
                raise NotImplementedError(f"build_generator: {k}={v!r} -- only plain beam search is implemented{hint}")
        gen_kwargs.pop("diverse_beam_strength", None)
        return dict(args, **gen_kwargs)

    def build_generator(self, **gen_kwargs):
        """SequenceGenerator from the reference's generator arguments (`generator_kwargs`)."""
        from .generator import SequenceGenerator
        if self.global_dict is None:
            raise ValueError(f"task {self.name}: initialize(global_dict) before building a generator")
        return SequenceGenerator(self.global_dict, **self.generator_kwargs(**gen_kwargs))

    def build_speech_generator(self, stats_npz_path: Optional[str] = None, **gen_kwargs):
        """AutoRegressiveSpeechGenerator from the reference's generator arguments (task/base.py:555-561): `max_iter` (default 1500) and
        `eos_prob_threshold` (default 0.5) are taken out, the rest (beam-search arguments of the shared default JSON among them) is
        ignored as there.  stats_npz_path: a local .npz with the `mean` / `std` of the global cepstral normalisation, or None (the
        reference's default is a URL, which nothing here fetches)."""
        from .generator import AutoRegressiveSpeechGenerator
        if self.global_dict is None:
            raise ValueError(f"task {self.name}: initialize(global_dict) before building a generator")
        max_iter = gen_kwargs.pop("max_iter", 1500)
        eos_prob_threshold = gen_kwargs.pop("eos_prob_threshold", 0.5)
        extra = {k: gen_kwargs.pop(k) for k in ("use_graph", "fused_step", "graph_cap") if k in gen_kwargs}
        return AutoRegressiveSpeechGenerator(self.global_dict, stats_npz_path=stats_npz_path, max_iter=max_iter,
                                             eos_prob_threshold=eos_prob_threshold, **extra)

    def sampling_generator(self, **gen_kwargs):
        """SequenceGenerator(search_strategy=Sampling(...)) from the reference's generator arguments: `sampling`, `sampling_topk`,
        `sampling_topp` (task/base.py:488-515, with its checks) and `seed` are taken out here, the rest goes through
        `generator_kwargs`.  One generator is kept per option set, so its captured step graphs -- and its stream of random
        numbers -- carry on over later batches.  `task.generator = task.sampling_generator(...)` makes `inference` sample."""
        from .generator import Sampling, SequenceGenerator
        if self.global_dict is None:
            raise ValueError(f"task {self.name}: initialize(global_dict) before building a generator")
        sampling = gen_kwargs.pop("sampling", True)
        topk, topp = gen_kwargs.pop("sampling_topk", -1), gen_kwargs.pop("sampling_topp", -1.0)
        seed = gen_kwargs.pop("seed", None)
        others = [gen_kwargs.get("diverse_beam_groups", -1) > 0, gen_kwargs.get("match_source_len", False),
                  gen_kwargs.get("diversity_rate", -1) > 0]
        if sampling and any(others):
            raise ValueError("Provided Search parameters are mutually exclusive.")
        assert topk < 0 or sampling, "--sampling-topk requires --sampling"
        assert topp < 0 or sampling, "--sampling-topp requires --sampling"
        if not sampling:
            raise ValueError("sampling_generator: sampling=False -- build_generator makes the beam-search generator")
        kw = self.generator_kwargs(**gen_kwargs)
        key = tuple(sorted((k, repr(v)) for k, v in dict(kw, sampling_topk=topk, sampling_topp=topp, seed=seed).items()))
        if key not in self._sampling_gens:
            self._sampling_gens[key] = SequenceGenerator(self.global_dict, search_strategy=Sampling(self.global_dict, topk, topp),
                                                         seed=seed, **kw)
        return self._sampling_gens[key]

    def diverse_generator(self, **gen_kwargs):
        """SequenceGenerator(search_strategy=DiverseBeamSearch(...) or DiverseSiblingsSearch(...)) from the reference's generator
        arguments: `diverse_beam_groups`, `diverse_beam_strength` (default 0.5) and `diversity_rate` are taken out here with the
        reference's exclusivity check and selection order (task/base.py:491-532: groups when > 0, else siblings when the rate is
        > -1), the rest goes through `generator_kwargs`.  One generator is kept per option set, so its captured step graphs carry
        on over later batches.  `task.generator = task.diverse_generator(...)` makes `inference` decode diversely."""
        from .generator import DiverseBeamSearch, DiverseSiblingsSearch, SequenceGenerator
        if self.global_dict is None:
            raise ValueError(f"task {self.name}: initialize(global_dict) before building a generator")
        groups, strength = gen_kwargs.pop("diverse_beam_groups", -1), gen_kwargs.pop("diverse_beam_strength", 0.5)
        rate = gen_kwargs.pop("diversity_rate", -1)
        if sum(int(bool(c)) for c in (gen_kwargs.get("sampling", False), groups > 0, gen_kwargs.get("match_source_len", False),
                                      rate > 0)) > 1:
            raise ValueError("Provided Search parameters are mutually exclusive.")
        if not (groups > 0 or rate > -1):
            raise ValueError("diverse_generator: neither diverse_beam_groups > 0 nor diversity_rate > -1 -- build_generator makes "
                             "the beam-search generator")
        kw = self.generator_kwargs(**gen_kwargs)
        chosen = dict(diverse_beam_groups=groups, diverse_beam_strength=strength) if groups > 0 else dict(diversity_rate=rate)
        key = tuple(sorted((k, repr(v)) for k, v in dict(kw, **chosen).items()))
        if key not in self._diverse_gens:
            strategy = DiverseBeamSearch(self.global_dict, groups, strength) if groups > 0 else \
                DiverseSiblingsSearch(self.global_dict, rate)
            self._diverse_gens[key] = SequenceGenerator(self.global_dict, search_strategy=strategy, **kw)
        return self._diverse_gens[key]

    @property
    def generator(self):
        """Built on first use from cfg.evaluation.generator_args (JSON) and cfg.constraint_range (text targets); an [AUDIO:...]
        target gets the autoregressive speech generator (`build_speech_generator`)."""
        if self._generator is None:
            gen_args = json.loads(self.cfg.evaluation.generator_args)
            if self.target_modality == ModalityType.TEXT:
                # closed-set tasks: the reference constrains every step with the text preprocessor's trie (task/base.py:236-240);
                # SequenceGenerator refuses a trie rather than generate free text
                gen_args["constraint_trie"] = self.general_preprocess.name2pre["text"].constraint_trie
                gen_args["constraint_range"] = self.cfg.constraint_range
            elif self.target_modality == ModalityType.AUDIO:
                self._generator = self.build_speech_generator(**gen_args)
                return self._generator
            elif self.target_modality is not None:
                raise NotImplementedError(f"task {self.name}: generation for {self.target_modality} targets is not implemented")
            self._generator = self.build_generator(**gen_args)
        return self._generator

    @generator.setter
    def generator(self, generator):
        self._generator = generator

    @property
    def scst_generator(self):
        """Built on first use from cfg.scst_args (task/base.py:249-253): every hypothesis of the beam is returned (SCST scores all K
        of a sentence); with "sampling": true the K rows are K independent samples (`sampling_generator`), and with
        "diverse_beam_groups" > 0 or "diversity_rate" > -1 they come from diverse decoding (`diverse_generator`)."""
        if self._scst_generator is None:
            args = json.loads(self.cfg.scst_args)
            args.setdefault("return_n_best", args.get("beam", 5))
            if args.get("sampling", False):
                self._scst_generator = self.sampling_generator(**args)
            elif args.get("diverse_beam_groups", -1) > 0 or args.get("diversity_rate", -1) > -1:
                self._scst_generator = self.diverse_generator(**args)
            else:
                args.pop("sampling", None)
                self._scst_generator = self.build_generator(**args)
        return self._scst_generator

    def inference(self, model, sample, **kwargs):
        """Beam search on `sample` (a collated batch); for TEXT targets every hypothesis gets `.text` through the task's text
        tokenizer (preprocessor/default/text.py:340-371).  As there, a sample with `prefix_tokens` has the sentence's prefix (its
        entries that are neither <pad> nor <eos>) cut from the front of `.tokens` before decoding; scores and positional scores
        keep the prefix positions.  An AUDIO target: the speech generator's SpeechGeneratorOutput list, untouched.  The model is left
        in eval mode."""
        model.eval()
        outputs = self.generator.generate(model, sample, **kwargs)
        if self.target_modality == ModalityType.TEXT:
            pre = self.general_preprocess.name2pre["text"]
            prefix = sample.get("prefix_tokens")
            for idx, single in enumerate(outputs):
                for hyp in (single if isinstance(single, list) else [single]):
                    if prefix is not None:
                        row = prefix[idx]
                        hyp.tokens = hyp.tokens[int((row.ne(self.global_dict.pad()) & row.ne(self.global_dict.eos())).sum()):]
                    hyp.text = pre.decode(hyp.tokens)
        return outputs


def collect_adaptor_name_from_tasks(tasks) -> Set[str]:
    names = set()
    for task in tasks:
        for template in task.templates:
            for slot in Instruction(template).slots:
                names.add(slot.get_attr("adaptor") if slot.has_attr("adaptor") else default_adaptor[slot.modality])
    return names
