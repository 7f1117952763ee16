"""MusicAVQA samples (reference dataloader/musicavqa.py:8-194): one free-text answer as the single option "(A)", fifteen
question types (modality x kind), the question's <placeholders> filled from `templ_values`, CLIP frame features and ImageBind
audio features sub-sampled or zero-padded to `max_feats`. The reference reads hard-coded cluster paths; here everything lies
under `args.data_root` (default "./data") as the NExT-QA reader's files do:
    musicavqa/avqa-{split}.json
    musicavqa/video/clipvitl14.pth
    musicavqa/audio_features_imagebind_10_frames/features/imagebind.pth     (max_feats rows of 1024 per clip)
    musicavqa/audio_features_imagebind/features/imagebind.pth               (one row per clip: audio_merge == "attention")
`templ_values` and `type` are list literals stored as strings: parsed with ast.literal_eval (the reference evals them).
Audio is padded with its own width (the reference pads with the video width, which cannot be concatenated to 1024-wide rows:
its padding branch only ever ran on features that were already `max_feats` long)."""
import ast
import json
import os
import re
from typing import Any, Dict, Tuple

import torch

from .base_dataset import BaseDataset
from .nextqa import sample_frames


class MusicAVQA(BaseDataset):
    QTYPES = {f"{m}_{k}": 1 + 5 * i + j
              for i, m in enumerate(("Audio", "Visual", "Audio-Visual"))
              for j, k in enumerate(("Temporal", "Existential", "Comparative", "Location", "Counting"))}

    def __init__(self, args: Any = None, tokenizer: Any = None, split: str = "train") -> None:
        super().__init__(args, tokenizer, split)
        root = os.path.join(getattr(args, "data_root", "./data"), "musicavqa")
        with open(os.path.join(root, f"avqa-{split}.json")) as f:
            self.data = json.load(f)
        self.audio = bool(getattr(args, "audio", False))
        self.audio_only = bool(getattr(args, "audio_only", False))
        self.one_audio_row = getattr(args, "audio_merge", None) == "attention"
        self.video_features, self.audio_features = {}, {}
        if not self.audio_only:
            self.video_features = torch.load(os.path.join(root, "video", "clipvitl14.pth"))
        if self.audio:
            folder = "audio_features_imagebind" if self.one_audio_row else "audio_features_imagebind_10_frames"
            self.audio_features = torch.load(os.path.join(root, folder, "features", "imagebind.pth"))
        self.answer_mapping = {0: "(A)"}
        self.num_options = 1
        self.qtype_mapping = dict(self.QTYPES)
        print(f"Num {split} data: {len(self.data)}")

    def _get_text(self, question: str, options) -> Dict[str, Any]:
        question = question.capitalize().strip()
        if not question.endswith("?"):
            question += "?"
        choices = "".join(f"{self.answer_mapping[i]} {options[i]}\n" for i in range(self.num_options))
        return {"q_text": f"Question: {question}\n", "o_text": "Choices: \n" + choices,
                "a_text": "Answer: The answer is ", "options": options}

    def _get_video(self, video_id: str) -> Tuple[torch.Tensor, int]:
        if video_id in self.video_features:
            feats = self.video_features[video_id].float()
        else:
            print(video_id, "video not found!")
            feats = torch.zeros(1, self.features_dim)
        return sample_frames(feats, self.max_feats)

    def _get_audio(self, audio_id: str) -> Tuple[torch.Tensor, int]:
        """(max_feats, 1024) and the number of real rows; with audio_merge == "attention" a shorter feature — the (1, 1024)
        row of the clip — is kept as it is and reported as max_feats long (reference musicavqa.py:146-150)."""
        if audio_id in self.audio_features:
            feats = self.audio_features[audio_id].float()
        else:
            print(audio_id, "audio not found!")
            feats = torch.zeros(1, self.audio_features_dim)
        if self.one_audio_row and feats.shape[0] <= self.max_feats:
            return feats, self.max_feats
        return sample_frames(feats, self.max_feats)

    def __getitem__(self, idx: int) -> Dict[str, Any]:
        item = self.data[idx]
        vid = item["video_id"]
        question = item["question_content"]
        answer_content = item.get("anser", "")                 # (the dataset's own spelling)
        values = ast.literal_eval(item["templ_values"])
        for i, name in enumerate(re.findall(r"<(.*?)>", question)):
            if i < len(values):
                question = question.replace(f"<{name}>", values[i], 1)
        kind = ast.literal_eval(item["type"])
        answer = 0
        text = self._get_text(question, [answer_content])
        text_id, label, video_start, video_index, label_mask, prefix_index = self._get_text_token(
            text, answer, options=text["options"])
        out = {"vid": vid}
        if not self.audio_only:
            out["video"], out["video_len"] = self._get_video(f"{vid}")
        out.update({"text": text, "text_id": text_id, "label": label, "video_start": video_start, "video_index": video_index})
        if self.audio:
            out["audio"], out["audio_len"] = self._get_audio(f"{vid}")
        out.update({"label_mask": label_mask, "qid": idx, "answer": answer, "qtype": self.qtype_mapping[f"{kind[0]}_{kind[1]}"],
                    "prefix_index": prefix_index})
        return out

    def __len__(self) -> int:
        return len(self.data)
