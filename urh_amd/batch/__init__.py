"""Many short captures in one pass (include/urhgpu.h "a batch of captures"; urh_amd/csrc/batch.hip).

A pass over one capture is all fixed cost below a few hundred thousand samples; a recording session is a directory of hundreds or
thousands of such captures.  DevicePipeline.iq_to_bits_batch packs them into ONE pinned staging buffer, uploads it with one copy, has
three launches demodulate and digitise all of them (a wavefront per capture), and fetches every capture's compact result blob with one
copy.  The results are HostBits made at the directory's offsets: no new result format.  Long captures still belong to passes and
streams -- a wavefront walks its capture serially --, so a capture of `long_from` samples or more is routed through the ordinary
iq_to_bits and takes its place in the sequence.

DevicePipeline.iq_to_bits_batch_auto opens the captures the way the reference opens each of its files: one more launch in front
(k_batch_noise, urh_amd/csrc/batch_auto.hip) runs AutoInterpretation.detect_noise_level on every capture, and the walk gates each capture
with its own threshold -- four launches and three read-backs whatever the number of captures.  detect_noise_levels is that first launch
alone.

DevicePipeline.iq_to_bits_batch_center also slices every capture with its OWN center (urh_amd/csrc/batch_center.hip): the captures are
demodulated into one buffer, one chain of kernels runs AutoInterpretation.detect_center on all of them, and the walk classifies each
capture through the thresholds of its center.  Where the device leaves a center to numpy (more bins than its pool holds, a tie between
the second and the third peak) the host settles it and ALL those captures are sliced again by one more call.  detect_centers is the chain
alone, qad_to_bits_batch the walk alone.

DevicePipeline.iq_to_bits_batch_records ends any of the three with the session's MESSAGES: one record per message (RSSI, first position,
ASK padding) queued behind the walk for all captures at once (urh_amd/csrc/batch_records.hip) -- three more launches and one more copy,
whatever the number of captures and of messages.  BatchBits.messages() is then what ProtocolAnalyzer.get_protocol_from_signal builds per file.

DevicePipeline.estimate_batch stands in front of all of them: AutoInterpretation.estimate of every capture -- modulation, samples per symbol,
center, tolerance, noise --, with the captures' message ranges from three launches (urh_amd/csrc/batch_estimate.hip: a wavefront per capture
follows segment_messages_from_magnitudes) and the messages of all captures pooled through the native calls estimators.estimate_dev makes for one
capture.  segment_messages_batch is the segmentation alone.

DevicePipeline.iq_to_bits_batch_psk is the batch of PSK captures (urh_amd/csrc/batch_psk.hip): ONE launch runs the Costas loop of every
capture -- a lane per capture, each from the known start state, nothing speculated -- into the demodulated buffer, and the route of
iq_to_bits_batch_center goes on from there (the center chain only when asked for, the qad-input walk, the records) with the parameters
recoded as FSK, whose noise value PSK shares.  The loop is serial: the device time follows the LONGEST capture of the batch, not their
number.  costas_demod_batch is that launch alone.  The entry points above keep refusing PSK and name this one.

DevicePipeline.iq_to_bits_batch_dc is any of the above over captures minus their own means -- the reference's DC correction, the default of
its receive path (urh_amd/csrc/batch_dc.hip): TWO launches in front correct every capture on the device, bit-equal with numpy's expression
(for float32 captures numpy's strictly sequential column sum, a lane per capture and column), and the matching batch runs on the corrected
buffer.  dc_correct_batch is those two launches alone; what it returns is the third input form of every batch method.  The entry points
above keep refusing dc_correction and name this one.

DevicePipeline.iq_to_bits_batch_each is the batch of a session whose transmitters are not alike (urh_amd/csrc/batch_each.hip): capture k is
demodulated, sliced and -- on request -- given its message records with params[k], from a table of K records and one shared threshold table
that travel in the batch's one upload.  One walk launch per modulation present (at most two), whatever the number of captures and of different
parameter sets.  params_from_estimates turns what estimate_batch returns into that list.
"""
from .center import TIE_POOL_COUNTS_PER_CAPTURE, batch_center_plan, center_thresholds, detect_centers
from .each import EACH_DTYPE, batch_plan_each, each_table, iq_to_bits_batch_each, params_from_estimates
from .estimate import ESTIMATE_SAMPLE_TYPES, MSG_GROUP, BatchEstimates, check_estimate_options, estimate_batch, segment_messages_batch
from .inputs import LONG_FROM_DEFAULT, per_capture, route
from .options import (as_fsk, check_batch_auto_options, check_batch_center_options, check_batch_dc_options, check_batch_each_options, check_batch_options,
                      check_batch_psk_options, check_batch_records_options, is_psk)
from .psk_dc import costas_demod_batch, dc_correct_batch
from .run import (BatchBits, detect_noise_levels, iq_to_bits_batch, iq_to_bits_batch_auto, iq_to_bits_batch_center, iq_to_bits_batch_dc, iq_to_bits_batch_psk,
                  iq_to_bits_batch_records, qad_to_bits_batch)
from .staging import batch_plan, batch_step, launch_counts
from .walk import FIRST_BLOB_BUFFER_BYTES, record_capacity
