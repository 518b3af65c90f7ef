"""A second, deliberately literal restatement of diverse (group) beam search as transformers 4.40.1 runs it for a batch of one (GenerationMixin._group_beam_search,
BeamSearchScorer with num_beam_groups = G, BeamHypotheses, HammingDiversityLogitsProcessor [ext]): flat tensors, one `current_tokens` vector, ONE scorer object that
holds G hypothesis sets and G done flags.  It shares no code with grounded_video_llm_amd/beam.py and follows HF's structure, not beam.py's; the CPU tests demand that
the two agree in ids, scores (as Python floats) and transition scores.  Not a test module itself.

model(list of generated ids) -> logits [vocab] stands for the language model: a beam's next-token logits are a pure function of what it generated."""
import torch


class Hypotheses:
    """BeamHypotheses(num_beams = group size)"""

    def __init__(self, size, length_penalty, early_stopping):
        self.size, self.length_penalty, self.early_stopping = size, length_penalty, early_stopping
        self.beams = []                                        # (score, ids tensor, ended by eos, beam-index trail)
        self.worst_score = 1e9

    def __len__(self):
        return len(self.beams)

    def add(self, hyp, sum_logprobs, generated_len, by_eos, trail):
        score = sum_logprobs / (generated_len ** self.length_penalty)
        if len(self) < self.size or score > self.worst_score:
            self.beams.append((score, hyp, by_eos, trail))
            if len(self) > self.size:
                sorted_next_scores = sorted([(s, idx) for idx, (s, _, _, _) in enumerate(self.beams)])
                del self.beams[sorted_next_scores[0][1]]
                self.worst_score = sorted_next_scores[1][0]
            else:
                self.worst_score = min(score, self.worst_score)

    def is_done(self, best_sum_logprobs, cur_len):
        if len(self) < self.size:
            return False
        if self.early_stopping is True:
            return True
        if self.early_stopping is False:
            highest_attainable_score = best_sum_logprobs / cur_len ** self.length_penalty
            return self.worst_score >= highest_attainable_score
        if self.length_penalty > 0.0:                          # "never" would need max_length here
            raise ValueError("early_stopping='never' with length_penalty > 0 needs max_length; not used by the reference")
        highest_attainable_score = best_sum_logprobs / cur_len ** self.length_penalty
        return self.worst_score >= highest_attainable_score


class Scorer:
    """BeamSearchScorer(batch_size = 1, num_beams, num_beam_groups)"""

    def __init__(self, num_beams, num_beam_groups, length_penalty, early_stopping, num_keep, max_length):
        self.num_beams, self.num_beam_groups, self.group_size = num_beams, num_beam_groups, num_beams // num_beam_groups
        self.num_keep, self.max_length = num_keep, max_length
        self._beam_hyps = [Hypotheses(self.group_size, length_penalty, early_stopping) for _ in range(num_beam_groups)]
        self._done = torch.tensor([False for _ in range(num_beam_groups)], dtype=torch.bool)

    @property
    def is_done(self):
        return bool(self._done.all())

    def process(self, input_ids, next_scores, next_tokens, next_indices, pad_token_id, eos_token_id, group_index):
        """input_ids [group_size, cur_len - 1] of the group; next_* [2 * group_size], best first"""
        cur_len = input_ids.shape[-1] + 1
        next_beam_scores = torch.zeros((self.group_size,), dtype=next_scores.dtype)
        next_beam_tokens = torch.zeros((self.group_size,), dtype=next_tokens.dtype)
        next_beam_indices = torch.zeros((self.group_size,), dtype=next_indices.dtype)
        if self._done[group_index]:
            next_beam_scores[:] = 0
            next_beam_tokens[:] = pad_token_id
            next_beam_indices[:] = 0
            return next_beam_scores, next_beam_tokens, next_beam_indices
        beam_idx = 0
        for beam_token_rank, (next_token, next_score, next_index) in enumerate(zip(next_tokens, next_scores, next_indices)):
            if eos_token_id is not None and next_token.item() == eos_token_id:
                if beam_token_rank >= self.group_size:
                    continue
                self._beam_hyps[group_index].add(input_ids[next_index].clone(), next_score.item(), cur_len, True, (int(next_index), beam_token_rank))
            else:
                next_beam_scores[beam_idx] = next_score
                next_beam_tokens[beam_idx] = next_token
                next_beam_indices[beam_idx] = next_index
                beam_idx += 1
            if beam_idx == self.group_size:
                break
        if beam_idx < self.group_size:
            raise ValueError("fewer than num_beams non-eos candidates among the top 2 x num_beams")
        self._done[group_index] = self._done[group_index] or self._beam_hyps[group_index].is_done(next_scores.max().item(), cur_len)
        return next_beam_scores, next_beam_tokens, next_beam_indices

    def finalize(self, input_ids, final_beam_scores, eos_token_id, hyp_scores_of):
        """-> [(ids list, score, transition scores)], the num_keep best over all groups; hyp_scores_of(entry) -> the transition scores of a pooled hypothesis"""
        for group_index, beam_hyp in enumerate(self._beam_hyps):
            if self._done[group_index]:
                continue
            for index_per_group in range(self.group_size):
                beam_id = group_index * self.group_size + index_per_group
                beam_hyp.add(input_ids[beam_id], final_beam_scores[beam_id].item(), input_ids[beam_id].shape[-1], False, (beam_id, None))
        candidate_beams = [beam for beam_hyp in self._beam_hyps for beam in beam_hyp.beams]
        sorted_hyps = sorted(candidate_beams, key=lambda x: x[0])
        out = []
        for _ in range(self.num_keep):
            score, ids, by_eos, trail = sorted_hyps.pop()
            ids = ids.tolist()
            ts = hyp_scores_of(trail)
            if by_eos and eos_token_id is not None and len(ids) < self.max_length:
                ids = ids + [eos_token_id]
            out.append((ids, score, ts[:len(ids)]))
        return out


def hamming(scores, current_tokens, group_start_idx, diversity_penalty, beam_group_idx):
    """HammingDiversityLogitsProcessor.__call__ for a batch of one"""
    if group_start_idx == 0:
        return scores
    vocab_size = scores.shape[-1]
    previous_group_tokens = current_tokens[:group_start_idx]
    previous_group_tokens = previous_group_tokens[(previous_group_tokens >= 0) & (previous_group_tokens < vocab_size)]     # an absent pad (-1) counts nowhere
    token_frequency = torch.bincount(previous_group_tokens, minlength=vocab_size)
    scores = scores.clone()
    scores -= torch.tensor(diversity_penalty, dtype=torch.float32) * token_frequency.to(torch.float32)
    return scores


def group_beam_search_ref(model, num_beams, num_beam_groups, diversity_penalty, max_new_tokens, eos_token_id, pad_token_id, length_penalty=1.0,
                          early_stopping=False, num_return=1):
    num_sub_beams = num_beams // num_beam_groups
    scorer = Scorer(num_beams, num_beam_groups, length_penalty, early_stopping, num_return, max_new_tokens)
    pad = -1 if pad_token_id is None else pad_token_id
    input_ids = torch.zeros((num_beams, 0), dtype=torch.long)
    beam_scores = torch.full((num_beams,), -1e9, dtype=torch.float32)
    beam_scores[::num_sub_beams] = 0
    trans = torch.zeros((num_beams, 0), dtype=torch.float32)   # what compute_transition_scores would gather: per beam, the processed score of each of its ids
    closed = {}                                                # transition scores of the hypotheses closed by eos, keyed by the scorer's trail
    step_no = 0
    while True:
        current_tokens = torch.zeros((num_beams,), dtype=torch.long)
        reordering_indices = torch.zeros((num_beams,), dtype=torch.long)
        logits = torch.stack([model(input_ids[b].tolist()) for b in range(num_beams)]).float()
        new_input_ids, new_trans = input_ids.clone(), torch.zeros((num_beams, trans.shape[1] + 1), dtype=torch.float32)
        for beam_group_idx in range(num_beam_groups):
            group_start_idx = beam_group_idx * num_sub_beams
            group_end_idx = min(group_start_idx + num_sub_beams, num_beams)
            group_size = group_end_idx - group_start_idx
            group_input_ids = input_ids[group_start_idx:group_end_idx]
            next_token_scores = torch.log_softmax(logits[group_start_idx:group_end_idx], dim=-1)
            vocab_size = next_token_scores.shape[-1]
            next_token_scores_processed = hamming(next_token_scores, current_tokens, group_start_idx, diversity_penalty, beam_group_idx)
            next_token_scores = next_token_scores_processed + beam_scores[group_start_idx:group_end_idx].unsqueeze(-1)
            next_token_scores = next_token_scores.view(group_size * vocab_size)
            next_token_scores, next_tokens = torch.topk(next_token_scores, 2 * group_size, dim=0, largest=True, sorted=True)
            next_indices = torch.div(next_tokens, vocab_size, rounding_mode="floor")
            next_tokens = next_tokens % vocab_size
            was_done = bool(scorer._done[beam_group_idx])
            # the scorer keys a hypothesis it closes by (beam, rank): remember what its transition scores would be
            for rank in range(2 * group_size):
                b, t = int(next_indices[rank]), int(next_tokens[rank])
                closed[(step_no, beam_group_idx, b, rank)] = trans[group_start_idx + b].tolist() + [float(next_token_scores_processed[b, t])]
            before = list(scorer._beam_hyps[beam_group_idx].beams)
            b_scores, b_tokens, b_idx = scorer.process(group_input_ids, next_token_scores, next_tokens, next_indices, pad, eos_token_id, beam_group_idx)
            # stamp the hypotheses this call added with the step and the group, so finalize can find their transition scores
            hy = scorer._beam_hyps[beam_group_idx]
            hy.beams = [e if any(e is o for o in before) else (e[0], e[1], e[2], (step_no, beam_group_idx) + tuple(e[3])) for e in hy.beams]
            beam_scores[group_start_idx:group_end_idx] = b_scores
            new_input_ids[group_start_idx:group_end_idx] = group_input_ids[b_idx]
            group_next = torch.cat([group_input_ids[b_idx], b_tokens.unsqueeze(-1)], dim=-1)
            current_tokens[group_start_idx:group_end_idx] = group_next[:, -1]
            for j in range(group_size):
                src = group_start_idx + int(b_idx[j])
                new_trans[group_start_idx + j, :-1] = trans[src]
                new_trans[group_start_idx + j, -1] = 0.0 if was_done else next_token_scores_processed[int(b_idx[j]), int(b_tokens[j])]
            reordering_indices[group_start_idx:group_end_idx] = group_start_idx + b_idx
        input_ids = torch.cat([new_input_ids, current_tokens.unsqueeze(-1)], dim=-1)
        trans = new_trans
        step_no += 1
        if scorer.is_done or input_ids.shape[-1] >= max_new_tokens:
            break

    def hyp_scores_of(trail):
        if len(trail) == 2:                                    # an open beam added by finalize: (beam, None)
            return trans[trail[0]].tolist()
        return closed[trail]
    res = scorer.finalize(input_ids, beam_scores, eos_token_id, hyp_scores_of)
    return res[0] if num_return == 1 else res
