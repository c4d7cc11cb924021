# Julia binding of librsys_hip.so (C ABI: include/rsys.h) -- thin `ccall` wrappers, 1:1 with the header: every entry point of
# the header is bound here; the test and parity hooks of include/rsys_debug.h (index-path read-back, in-process rank group, per-kernel
# access) are not part of the boundary and are not bound.  tests/test_julia_binding.py parses the `ccall` tuples and the two struct mirrors below and checks
# names, arity and C types against include/rsys.h (Julia itself cannot run in the build image).
#
# NOT EXECUTED in the build container (Julia is absent from the image, SURVEY.md 8(c)); it is the stub a
# maintainer adds so that notebooks/Training/run.jl:70 (`julia rungpu.jl`, which remote-launches torchrun
# transformer.py) can call the HIP path in-process instead.  Host arrays are kept alive with GC.@preserve
# for the duration of each call; the library owns all device memory.
module RsysHIP

const LIB = joinpath(@__DIR__, "..", "recommendersystem_amd", "librsys_hip.so")

# RsysConfig.dtype (rsys.h RSYS_DTYPE_*): fp32 parity mode, the bf16 autocast arithmetic, or bf16 with the blocks' linears on
# tensor-wise scaled fp8 operands -- what transformer.py:671-676 gets from torchao's convert_to_float8_training
const DTYPE_FP32 = Int32(0); const DTYPE_BF16 = Int32(1); const DTYPE_FP8 = Int32(2)

struct RsysConfig              # mirrors rsys_config (field order and types as in rsys.h)
    num_layers::Int32; num_heads::Int32; num_kv_heads::Int32; embed_dim::Int32; intermediate_dim::Int32
    max_sequence_length::Int32
    vocab_0::Int32; vocab_1::Int32
    vocab_status::Int32; vocab_gender::Int32; vocab_source::Int32
    metadata_dim::Int32
    min_ts::Float64; max_ts::Float64
    rating_mean::Float32; rating_std::Float32; mask_rate::Float32
    mask_topk::Int32; finetune::Int32; finetune_metric::Int32
    dtype::Int32; max_rows::Int32
    lora_dropout::Float32
    table_shard_rank::Int32; table_shard_world::Int32     # row-sharded item table (world 0 = replicated)
    sampled_negatives::Int32                               # sampled soft-max over the local classes (0 = full)
end

struct RsysBatch               # mirrors rsys_batch
    rows::Int32
    userid::Ptr{Int32}; token_mask_ids::Ptr{Int32}; gender::Ptr{Int32}; source::Ptr{Int32}
    matchedid::Ptr{Int32}; status::Ptr{Int32}
    time::Ptr{Float64}; rating::Ptr{Float32}; progress::Ptr{Float32}
    label::NTuple{6,Ptr{Float32}}; weight::NTuple{6,Ptr{Float32}}; position::NTuple{6,Ptr{Int32}}
    watch_mask::Ptr{UInt8}; rating_mask::Ptr{UInt8}; rope_input_pos::Ptr{Int32}
end

function last_error()
    buf = Vector{UInt8}(undef, 2048)
    ccall((:rsys_last_error, LIB), Csize_t, (Ptr{UInt8}, Csize_t), buf, length(buf))
    unsafe_string(pointer(buf))
end
check(rc) = rc == 0 ? nothing : error("rsys error $rc: $(last_error())")

mutable struct Model; h::Ptr{Cvoid}; end
mutable struct Optimizer; h::Ptr{Cvoid}; end
mutable struct Comm; h::Ptr{Cvoid}; world::Int; end

function Model(cfg::RsysConfig, device::Integer)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rsys_model_create, LIB), Int32, (Ref{RsysConfig}, Int32, Ref{Ptr{Cvoid}}), cfg, device, h))
    m = Model(h[]); finalizer(x -> ccall((:rsys_model_destroy, LIB), Int32, (Ptr{Cvoid},), x.h), m); m
end
init_weights!(m::Model, seed::Integer) = check(ccall((:rsys_model_init_random, LIB), Int32, (Ptr{Cvoid}, UInt64), m.h, seed))
function load_pretrained_embeddings!(m::Model, W::Matrix{Float32})   # W is (M, V) column-major = (V, M) row-major (transformer.jl:58)
    GC.@preserve W check(ccall((:rsys_model_load_metadata, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64),
                               m.h, W, size(W, 2), size(W, 1)))
end
function set_parameter!(m::Model, name::String, x::Array{Float32})
    GC.@preserve x check(ccall((:rsys_param_set, LIB), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float32}, Int64), m.h, name, x, length(x)))
end
function get_parameter!(m::Model, name::String, out::Array{Float32})
    GC.@preserve out check(ccall((:rsys_param_get, LIB), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float32}, Int64), m.h, name, out, length(out)))
    out
end
function upload!(m::Model, b::RsysBatch)    # caller wraps this in GC.@preserve of the arrays b points to
    check(ccall((:rsys_batch_upload, LIB), Int32, (Ptr{Cvoid}, Ref{RsysBatch}), m.h, b))
end
# the next batch beside the running step (second staging buffer + copy stream), then made the resident one: enqueue the step,
# prefetch!, read the losses, swap_batch!
function prefetch!(m::Model, b::RsysBatch)  # caller wraps this in GC.@preserve of the arrays b points to
    check(ccall((:rsys_batch_prefetch, LIB), Int32, (Ptr{Cvoid}, Ref{RsysBatch}), m.h, b))
end
swap_batch!(m::Model) = check(ccall((:rsys_batch_swap, LIB), Int32, (Ptr{Cvoid},), m.h))
function forward_backward!(m::Model, evaluate::Bool, task_w::NTuple{4,Float32}, grad_scale::Float32, seed::UInt64, step::UInt64)
    tw = Ref(task_w)
    check(ccall((:rsys_forward_backward, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Float32}, Float32, UInt64, UInt64),
                m.h, evaluate ? 1 : 0, tw, grad_scale, seed, step))
end
function losses(m::Model)
    lo = Vector{Float32}(undef, 12); ws = Vector{Float32}(undef, 4)
    check(ccall((:rsys_losses_get, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), m.h, lo, ws))
    lo, ws
end

# losses without a host wait per step (transformer.py:245-262 accumulates on the device): park, then read every parked step at once
push_losses!(m::Model) = check(ccall((:rsys_losses_push, LIB), Int32, (Ptr{Cvoid},), m.h))
function drain_losses(m::Model, cap::Integer = 1024)
    lo = Matrix{Float32}(undef, 12, cap); ws = Matrix{Float32}(undef, 4, cap); n = Ref{Int32}(0)
    GC.@preserve lo ws check(ccall((:rsys_losses_drain, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Int32, Ref{Int32}), m.h, lo, ws, cap, n))
    lo[:, 1:n[]], ws[:, 1:n[]]
end

set_deterministic!(m::Model, on::Bool = true) = check(ccall((:rsys_model_set_deterministic, LIB), Int32, (Ptr{Cvoid}, Int32), m.h, on ? 1 : 0))

# inference forward (model.py:531-538): task 0 = retrieval, 1 = ranking; `tokens` = flat token indices (0-based) to report
function infer_select(m::Model, task::Integer, tokens::Vector{Int32}, D::Integer)
    out = task == 0 ? Matrix{Float32}(undef, D, length(tokens)) : Vector{Float32}(undef, length(tokens))
    GC.@preserve tokens out check(ccall((:rsys_infer_select, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Int32}, Int64, Ptr{Float32}, Int64),
                                        m.h, task, tokens, length(tokens), out, length(out)))
    out
end

# adapter bank of a base model (Finetune/embed.py:180-255: four LoRA adapters on one trunk): tensors by state-dict name into slot
# 0 .. 7 (0-based, as the C ABI counts them), then one forward with a slot (or -1 = base model) per batch row
const ADAPTER_SLOTS = 8
function set_adapter!(m::Model, slot::Integer, name::String, x::Array{Float32})
    GC.@preserve x check(ccall((:rsys_adapter_set, LIB), Int32, (Ptr{Cvoid}, Int32, Cstring, Ptr{Float32}, Int64), m.h, slot, name, x, length(x)))
end
function get_adapter!(m::Model, slot::Integer, name::String, out::Array{Float32})
    GC.@preserve out check(ccall((:rsys_adapter_get, LIB), Int32, (Ptr{Cvoid}, Int32, Cstring, Ptr{Float32}, Int64), m.h, slot, name, out, length(out)))
    out
end
clear_adapter!(m::Model, slot::Integer) = check(ccall((:rsys_adapter_clear, LIB), Int32, (Ptr{Cvoid}, Int32), m.h, slot))
function adapter_slots(m::Model)
    mask = Ref{Int32}(0)
    check(ccall((:rsys_adapter_slots, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}), m.h, mask))
    [s for s in 0:ADAPTER_SLOTS-1 if (mask[] >> s) & 1 == 1]
end
function infer_select_adapters(m::Model, task::Integer, row_adapter::Vector{Int32}, tokens::Vector{Int32}, D::Integer)
    out = task == 0 ? Matrix{Float32}(undef, D, length(tokens)) : Vector{Float32}(undef, length(tokens))
    GC.@preserve row_adapter tokens out check(ccall((:rsys_infer_select_adapters, LIB), Int32,
                                                    (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int32}, Int64, Ptr{Float32}, Int64),
                                                    m.h, task, row_adapter, tokens, length(tokens), out, length(out)))
    out
end
# the same on packed rows (rsys.h: rsys_infer_select_tiles): tile_adapter (ceil(S / 32), rows) column-major = [rows][ceil(S / 32)], a slot or
# -1 per 32 interactions of a row; `nothing` runs the base model
function infer_select_tiles(m::Model, task::Integer, tile_adapter::Union{Matrix{Int32},Nothing}, tokens::Vector{Int32}, D::Integer)
    out = task == 0 ? Matrix{Float32}(undef, D, length(tokens)) : Vector{Float32}(undef, length(tokens))
    ta = tile_adapter === nothing ? Ptr{Int32}(C_NULL) : pointer(tile_adapter)
    GC.@preserve tile_adapter tokens out check(ccall((:rsys_infer_select_tiles, LIB), Int32,
                                                     (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int32}, Int64, Ptr{Float32}, Int64),
                                                     m.h, task, ta, tokens, length(tokens), out, length(out)))
    out
end

# Training through the adapter bank (rsys.h: rsys_adapter_train_enable ...; Finetune/run.jl:9-13 as one pass): row r of the resident
# batch runs with slot row_slot[r] on task row_task[r] = medium * 2 + metric (-1 / -1: base model, no loss)
function batch_rows(m::Model)
    n = Ref{Int32}(0)
    check(ccall((:rsys_batch_rows, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}), m.h, n))
    Int(n[])
end
# Inference on trimmed rows (rsys.h: rsys_batch_upload_trimmed ...): `b` keeps the row stride max_sequence_length, columns [1, row_len] of
# every row become the resident batch; the rest of each row must be padding (userid 0)
function batch_upload_trimmed(m::Model, b::RsysBatch, row_len::Integer)
    check(ccall((:rsys_batch_upload_trimmed, LIB), Int32, (Ptr{Cvoid}, Ref{RsysBatch}, Int32), m.h, b, row_len))
end
function batch_row_length(m::Model)
    n = Ref{Int32}(0)
    check(ccall((:rsys_batch_row_length, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}), m.h, n))
    Int(n[])
end
serving_pack!(m::Model, on::Bool) = check(ccall((:rsys_serving_pack_set, LIB), Int32, (Ptr{Cvoid}, Int32), m.h, on ? 1 : 0))
function serving_pack(m::Model)   # the retrieval stage of the two render calls packs several users into a row
    on = Ref{Int32}(0)
    check(ccall((:rsys_serving_pack_get, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}), m.h, on))
    on[] != 0
end
serving_pack_ranking!(m::Model, on::Bool) = check(ccall((:rsys_serving_pack_ranking_set, LIB), Int32, (Ptr{Cvoid}, Int32), m.h, on ? 1 : 0))
function serving_pack_ranking(m::Model)   # render_request_full packs its K/V-cache store rows (several histories per row)
    on = Ref{Int32}(0)
    check(ccall((:rsys_serving_pack_ranking_get, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}), m.h, on))
    on[] != 0
end
serving_compact_top!(m::Model, on::Bool) = check(ccall((:rsys_serving_compact_top_set, LIB), Int32, (Ptr{Cvoid}, Int32), m.h, on ? 1 : 0))
function serving_compact_top(m::Model)   # inference passes run the last layer only where its outputs are read
    on = Ref{Int32}(0)
    check(ccall((:rsys_serving_compact_top_get, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}), m.h, on))
    on[] != 0
end
serving_trim!(m::Model, on::Bool) = check(ccall((:rsys_serving_trim_set, LIB), Int32, (Ptr{Cvoid}, Int32), m.h, on ? 1 : 0))
function serving_trim(m::Model)
    on = Ref{Int32}(0)
    check(ccall((:rsys_serving_trim_get, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}), m.h, on))
    on[] != 0
end
adapter_train_enable(m::Model, dropout::Real) = check(ccall((:rsys_adapter_train_enable, LIB), Int32, (Ptr{Cvoid}, Float32), m.h, dropout))
function adapter_forward_backward(m::Model, evaluate::Bool, row_slot::Vector{Int32}, row_task::Vector{Int32}, grad_scale::Real, seed::Integer, step::Integer)
    GC.@preserve row_slot row_task check(ccall((:rsys_adapter_forward_backward, LIB), Int32,
                                               (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int32}, Float32, UInt64, UInt64),
                                               m.h, evaluate ? 1 : 0, row_slot, row_task, grad_scale, seed, step))
end
# the same on packed rows (rsys.h: rsys_adapter_forward_backward_packed): segments (5, n_seg) column-major = [n_seg][5] =
# (row, first_column, columns, slot, task), all 0-based as in the C ABI
function adapter_forward_backward_packed(m::Model, evaluate::Bool, segments::Matrix{Int32}, grad_scale::Real, seed::Integer, step::Integer)
    size(segments, 1) == 5 || throw(ArgumentError("segments is (5, n_seg)"))
    GC.@preserve segments check(ccall((:rsys_adapter_forward_backward_packed, LIB), Int32,
                                      (Ptr{Cvoid}, Int32, Ptr{Int32}, Int32, Float32, UInt64, UInt64),
                                      m.h, evaluate ? 1 : 0, segments, size(segments, 2), grad_scale, seed, step))
end
function adapter_grad!(m::Model, slot::Integer, name::String, out::Array{Float32})
    GC.@preserve out check(ccall((:rsys_adapter_grad_get, LIB), Int32, (Ptr{Cvoid}, Int32, Cstring, Ptr{Float32}, Int64), m.h, slot, name, out, length(out)))
    out
end
adapter_zero_grad(m::Model) = check(ccall((:rsys_adapter_zero_grad, LIB), Int32, (Ptr{Cvoid},), m.h))
# per_slot: 3 x n_slots (active, lr factor, max_norm per column); returns the slots' gradient norms
function adapter_adamw_step(m::Model, lr0::Real, beta1::Real, beta2::Real, eps::Real, wd::Real, per_slot::Matrix{Float32})
    n = size(per_slot, 2)
    norms = Vector{Float32}(undef, n)
    GC.@preserve per_slot norms check(ccall((:rsys_adapter_adamw_step, LIB), Int32,
                                            (Ptr{Cvoid}, Float32, Float32, Float32, Float32, Float32, Ptr{Float32}, Int32, Ptr{Float32}),
                                            m.h, lr0, beta1, beta2, eps, wd, per_slot, n, norms))
    norms
end
function adapter_adamw_state!(m::Model, slot::Integer, name::String, exp_avg::Array{Float32}, exp_avg_sq::Array{Float32})
    step = Ref{Int32}(0)
    GC.@preserve exp_avg exp_avg_sq check(ccall((:rsys_adapter_adamw_state_get, LIB), Int32,
                                                (Ptr{Cvoid}, Int32, Cstring, Ptr{Float32}, Ptr{Float32}, Int64, Ref{Int32}),
                                                m.h, slot, name, exp_avg, exp_avg_sq, length(exp_avg), step))
    step[]
end
function set_adapter_adamw_state!(m::Model, slot::Integer, name::String, exp_avg::Array{Float32}, exp_avg_sq::Array{Float32}, step::Integer)
    GC.@preserve exp_avg exp_avg_sq check(ccall((:rsys_adapter_adamw_state_set, LIB), Int32,
                                                (Ptr{Cvoid}, Int32, Cstring, Ptr{Float32}, Ptr{Float32}, Int64, Int32),
                                                m.h, slot, name, exp_avg, exp_avg_sq, length(exp_avg), step))
end

# Full-length ranking through a per-user K/V cache of the history (rsys.h: rsys_rank_cache_*).  row_adapter may be `nothing` (base model).
rank_cache_reserve(m::Model, n_slots::Integer) = check(ccall((:rsys_rank_cache_reserve, LIB), Int32, (Ptr{Cvoid}, Int32), m.h, n_slots))
function rank_cache_store(m::Model, row_adapter::Union{Nothing, Vector{Int32}}, n_hist::Vector{Int32}, slot::Vector{Int32})
    ra = row_adapter === nothing ? Ptr{Int32}(C_NULL) : pointer(row_adapter)
    GC.@preserve row_adapter n_hist slot check(ccall((:rsys_rank_cache_store, LIB), Int32, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
                                                     m.h, ra, n_hist, slot))
end
function rank_cache_candidates(m::Model, row_adapter::Union{Nothing, Vector{Int32}}, slot::Vector{Int32}, n_cand::Vector{Int32})
    out = Vector{Float32}(undef, sum(n_cand))
    ra = row_adapter === nothing ? Ptr{Int32}(C_NULL) : pointer(row_adapter)
    GC.@preserve row_adapter slot n_cand out check(ccall((:rsys_rank_cache_candidates, LIB), Int32,
                                                         (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}), m.h, ra, slot, n_cand, out))
    out
end
# The same two passes on packed rows (rsys.h: several users per row, one segment of whole 64-token tiles each).  seg: 4 x n_seg Int32,
# column i = (row, first_column, n_hist | n_cand, slot) of segment i, zero-based as in the C ABI; seg_adapter may be `nothing`.
function rank_cache_store_packed(m::Model, seg_adapter::Union{Nothing, Vector{Int32}}, seg::Matrix{Int32})
    sa = seg_adapter === nothing ? Ptr{Int32}(C_NULL) : pointer(seg_adapter)
    GC.@preserve seg_adapter seg check(ccall((:rsys_rank_cache_store_packed, LIB), Int32, (Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Int32}),
                                             m.h, sa, size(seg, 2), seg))
end
function rank_cache_candidates_packed(m::Model, seg_adapter::Union{Nothing, Vector{Int32}}, seg::Matrix{Int32})
    out = Vector{Float32}(undef, sum(seg[3, :]))
    sa = seg_adapter === nothing ? Ptr{Int32}(C_NULL) : pointer(seg_adapter)
    GC.@preserve seg_adapter seg out check(ccall((:rsys_rank_cache_candidates_packed, LIB), Int32,
                                                 (Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Float32}), m.h, sa, size(seg, 2), seg, out))
    out
end

function create_optimizer(m::Model; lr = 1f-4, betas = (0.9f0, 0.95f0), eps = 1f-8, weight_decay = 0.1f0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rsys_adamw_create, LIB), Int32, (Ptr{Cvoid}, Float32, Float32, Float32, Float32, Float32, Ref{Ptr{Cvoid}}),
                m.h, lr, betas[1], betas[2], eps, weight_decay, h))
    Optimizer(h[])
end
step!(o::Optimizer; lr_factor = 1f0, clip = 1f0, grad_div = 1f0) =
    check(ccall((:rsys_adamw_step, LIB), Int32, (Ptr{Cvoid}, Float32, Float32, Float32), o.h, lr_factor, clip, grad_div))
# (beyond the reference, opt-in) ZeRO-1: moments for this rank's 1/world of the parameters; step_zero1! replaces allreduce_grads! + step!
set_zero1!(o::Optimizer, rank::Integer, world::Integer) =
    check(ccall((:rsys_adamw_set_zero1, LIB), Int32, (Ptr{Cvoid}, Int32, Int32), o.h, rank, world))
step_zero1!(o::Optimizer, c; lr_factor = 1f0, clip = 1f0, grad_div = 1f0) =
    check(ccall((:rsys_adamw_step_zero1, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Float32, Float32, Float32), o.h, c.h, lr_factor, clip, grad_div))

function unique_id()
    id = Vector{UInt8}(undef, 128)
    check(ccall((:rsys_comm_unique_id, LIB), Int32, (Ptr{UInt8},), id)); id
end
function Comm(id::Vector{UInt8}, rank::Integer, world::Integer, device::Integer)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rsys_comm_init, LIB), Int32, (Ptr{UInt8}, Int32, Int32, Int32, Ref{Ptr{Cvoid}}), id, rank, world, device, h))
    Comm(h[], world)
end
self_test(c::Comm) = check(ccall((:rsys_self_test, LIB), Int32, (Ptr{Cvoid},), c.h))
allreduce_grads!(m::Model, c::Comm) = check(ccall((:rsys_allreduce_grads, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), m.h, c.h))
# arm the early gradient buckets for the next backward (the last micro-step of an optimizer step)
set_split_table_reduce!(m::Model, on::Bool=true) = check(ccall((:rsys_model_set_split_table_reduce, LIB), Int32, (Ptr{Cvoid}, Int32), m.h, on ? 1 : 0))
begin_grad_sync!(m::Model, c::Comm) = check(ccall((:rsys_set_grad_sync, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), m.h, c.h))

# row-sharded item table (rsys_config.table_shard_world >= 1): the communicator of the row exchange and the vocabulary-parallel
# cross entropy, and the table rows [lo, hi) this model holds
set_shard_comm!(m::Model, c::Comm) = check(ccall((:rsys_model_set_shard_comm, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), m.h, c.h))
function table_rows(m::Model)
    lo = Ref{Int64}(0); hi = Ref{Int64}(0)
    check(ccall((:rsys_table_rows, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), m.h, lo, hi)); (lo[], hi[])
end


# ---- lifetime, library
version() = unsafe_string(ccall((:rsys_version, LIB), Cstring, ()))
function device_count()
    n = Ref{Int32}(0); check(ccall((:rsys_device_count, LIB), Int32, (Ref{Int32},), n)); Int(n[])
end
synchronize() = check(ccall((:rsys_device_synchronize, LIB), Int32, ()))
destroy!(m::Model) = (m.h == C_NULL || check(ccall((:rsys_model_destroy, LIB), Int32, (Ptr{Cvoid},), m.h)); m.h = C_NULL; nothing)
destroy!(o::Optimizer) = (o.h == C_NULL || check(ccall((:rsys_adamw_destroy, LIB), Int32, (Ptr{Cvoid},), o.h)); o.h = C_NULL; nothing)
destroy!(c::Comm) = (c.h == C_NULL || check(ccall((:rsys_comm_destroy, LIB), Int32, (Ptr{Cvoid},), c.h)); c.h = C_NULL; nothing)

# ---- parameters (state-dict names of transformer.model.py:346-359)
random_pretrained_embeddings!(m::Model, seed::Integer) = check(ccall((:rsys_model_random_metadata, LIB), Int32, (Ptr{Cvoid}, UInt64), m.h, seed))
function set_rope!(m::Model, c::Matrix{Float32}, s::Matrix{Float32})   # (head_dim / 2, n_pos) column-major = (n_pos, head_dim / 2) row-major
    GC.@preserve c s check(ccall((:rsys_model_set_rope, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Int64), m.h, c, s, size(c, 2)))
end
function param_count(m::Model)
    n = Ref{Int32}(0); check(ccall((:rsys_param_count, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}), m.h, n)); Int(n[])
end
function param_info(m::Model, i::Integer)            # i is 0-based like the C ABI
    name = Vector{UInt8}(undef, 256); shape = Vector{Int64}(undef, 2); nd = Ref{Int32}(0); tr = Ref{Int32}(0)
    GC.@preserve name shape check(ccall((:rsys_param_info, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{UInt8}, Csize_t, Ptr{Int64}, Ref{Int32}, Ref{Int32}),
                                        m.h, i, name, length(name), shape, nd, tr))
    (unsafe_string(pointer(name)), nd[] == 1 ? (shape[1],) : (shape[1], shape[2]), tr[] != 0)
end
function grad!(m::Model, name::String, out::Array{Float32})
    GC.@preserve out check(ccall((:rsys_grad_get, LIB), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float32}, Int64), m.h, name, out, length(out)))
    out
end
zero_grad!(m::Model) = check(ccall((:rsys_zero_grad, LIB), Int32, (Ptr{Cvoid},), m.h))
refresh_shadow!(m::Model) = check(ccall((:rsys_refresh_shadow, LIB), Int32, (Ptr{Cvoid},), m.h))
function grad_buffer(m::Model)
    p = Ref{Ptr{Cvoid}}(C_NULL); n = Ref{Int64}(0)
    check(ccall((:rsys_grad_buffer, LIB), Int32, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Int64}), m.h, p, n)); (p[], n[])
end
function param_buffer(m::Model)
    p = Ref{Ptr{Cvoid}}(C_NULL); n = Ref{Int64}(0)
    check(ccall((:rsys_param_buffer, LIB), Int32, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Int64}), m.h, p, n)); (p[], n[])
end

# ---- clip, heads, serving
function clip_grad_norm!(m::Model, max_norm::Real)    # transformer.py:273
    out = Ref{Float32}(0f0)
    check(ccall((:rsys_clip_grad_norm, LIB), Int32, (Ptr{Cvoid}, Float32, Ref{Float32}), m.h, max_norm, out)); out[]
end
function head_rows(m::Model)
    out = Vector{Int32}(undef, 4)
    GC.@preserve out check(ccall((:rsys_head_rows_get, LIB), Int32, (Ptr{Cvoid}, Ptr{Int32}), m.h, out)); out
end
function item_table(m::Model, V::Integer, D::Integer)  # register.py:27-33: (D, V) column-major = (V, D) row-major
    out = Matrix{Float32}(undef, D, V)
    GC.@preserve out check(ccall((:rsys_item_table, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}, Int64), m.h, out, length(out))); out
end
# retrieval candidates on the device (Finetune/embed.jl:86-90 + Inference/render.jl:240-333's scoring, masking and sortperm): Q is
# (D, n_queries) column-major = (n_queries, D) row-major; `group` (0-based, one per query) or nothing (each query its own group); `prior`
# (V_m, n_groups) or nothing; `excl` one Vector{Int32} of 0-based medium-local ids per group, or nothing.  Returns (ids, scores, counts):
# (k, n_groups) 0-based medium-local ids (-1 past counts[g]), their scores (-Inf past counts[g]), admissible count per group.
function retrieve_topk(m::Model, medium::Integer, Q::Matrix{Float32}, k::Integer; group = nothing, n_groups::Integer = size(Q, 2),
                       prior = nothing, excl = nothing)
    g = group === nothing ? Ptr{Int32}(C_NULL) : Vector{Int32}(group)
    p = prior === nothing ? Ptr{Float32}(C_NULL) : Matrix{Float32}(prior)
    off = excl === nothing ? Ptr{Int64}(C_NULL) : Int64[0; cumsum(Int64[length(e) for e in excl])]
    xid = excl === nothing ? Ptr{Int32}(C_NULL) : Int32[reduce(vcat, excl; init = Int32[])...]
    ids = Matrix{Int32}(undef, k, n_groups); scores = Matrix{Float32}(undef, k, n_groups); counts = Vector{Int32}(undef, n_groups)
    GC.@preserve Q g p off xid ids scores counts check(ccall((:rsys_retrieve_topk, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float32}, Int64, Ptr{Int32}, Int32, Ptr{Float32}, Ptr{Int64}, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Float32}, Ptr{Int32}),
        m.h, medium, Q, size(Q, 2), g, n_groups, p, off, xid, k, ids, scores, counts))
    ids, scores, counts
end
# finetune evaluation (Finetune/regress.jl:193-266): per query (column of Q) the rank of its target among the admissible items (0 when
# the target is excluded) and the target's log-probability; targets and exclusion ids are 0-based medium-local, excl one vector per query
function retrieve_target_rank(m::Model, medium::Integer, Q::Matrix{Float32}, targets; excl = nothing)
    t = Vector{Int32}(targets)
    off = excl === nothing ? Ptr{Int64}(C_NULL) : Int64[0; cumsum(Int64[length(e) for e in excl])]
    xid = excl === nothing ? Ptr{Int32}(C_NULL) : Int32[reduce(vcat, excl; init = Int32[])...]
    rank = Vector{Int32}(undef, size(Q, 2)); logp = Vector{Float32}(undef, size(Q, 2))
    GC.@preserve Q t off xid rank logp check(ccall((:rsys_retrieve_target_rank, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float32}, Int64, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}),
        m.h, medium, Q, size(Q, 2), t, off, xid, rank, logp))
    rank, logp
end
# whole retrieval requests (Inference/render.jl:240-331, `retrieval(state)`): the serving tables are loaded onto the device once, then
# retrieve_request needs only the users' embeddings, their list items and the selected items.  kind: 0 = "{m}.dependencies",
# 1 = "{m}.recaps", 2 = "{m}.adaptations"; 0-based CSC arrays, or colptr = nothing to clear the table.
function retrieve_relations_set(m::Model, medium::Integer, kind::Integer, n_rows::Integer, n_cols::Integer, colptr, rowval, nzval)
    cp = colptr === nothing ? Ptr{Int64}(C_NULL) : Vector{Int64}(colptr)
    rv = colptr === nothing ? Ptr{Int32}(C_NULL) : Vector{Int32}(rowval)
    nz = colptr === nothing ? Ptr{Float32}(C_NULL) : Vector{Float32}(nzval)
    colptr === nothing || (length(cp) == n_cols + 1 && length(rv) >= cp[end] && length(nz) >= cp[end]) ||
        error("retrieve_relations_set: CSC arrays do not match n_cols / colptr")
    GC.@preserve cp rv nz check(ccall((:rsys_retrieve_relations_set, LIB), Int32,
        (Ptr{Cvoid}, Int32, Int32, Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float32}), m.h, medium, kind, n_rows, n_cols, cp, rv, nz))
end
# a SparseMatrixCSC as it is (relations["$m.dependencies"] etc.), or nothing to clear: colptr .- 1, rowval .- 1
set_relations!(m::Model, medium::Integer, kind::Integer, A) = A === nothing ?
    retrieve_relations_set(m, medium, kind, 0, 0, nothing, nothing, nothing) :
    retrieve_relations_set(m, medium, kind, size(A, 1), size(A, 2), A.colptr .- 1, A.rowval .- 1, A.nzval)
# item_similarity["embeddings.$m"] (dim, V_m) and item_similarity["crossproject.$m"] (dim, dim) or nothing, in their own memory layout
function retrieve_similarity_set(m::Model, medium::Integer, emb, crossproject = nothing)
    e = emb === nothing ? Ptr{Float32}(C_NULL) : Matrix{Float32}(emb)
    c = (emb === nothing || crossproject === nothing) ? Ptr{Float32}(C_NULL) : Matrix{Float32}(crossproject)
    dim = emb === nothing ? 0 : size(e, 1)
    GC.@preserve e c check(ccall((:rsys_retrieve_similarity_set, LIB), Int32, (Ptr{Cvoid}, Int32, Int64, Ptr{Float32}, Ptr{Float32}),
        m.h, medium, dim, e, c))
end
# released items of the medium as a Bool / UInt8 mask over the 0-based ids (length V_m), or nothing: every item released
function retrieve_released_set(m::Model, medium::Integer, mask = nothing)
    x = mask === nothing ? Ptr{UInt8}(C_NULL) : Vector{UInt8}(mask)
    GC.@preserve x check(ccall((:rsys_retrieve_released_set, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{UInt8}), m.h, medium, x))
end
# query weights of the NEXT request call on the model (rsys_query_weights_set): one finite Float32 per user / per selected item in the
# call's order, or nothing (unweighted for that kind; both nothing clears).  retrieve_request, retrieve_window, rank_request,
# render_request, render_request_full and render_items consume them, on success and on error alike.
function query_weights_set(m::Model, user_w = nothing, sel_w = nothing)
    u = (user_w === nothing || isempty(user_w)) ? Ptr{Float32}(C_NULL) : Vector{Float32}(user_w)
    s = (sel_w === nothing || isempty(sel_w)) ? Ptr{Float32}(C_NULL) : Vector{Float32}(sel_w)
    nu = u isa Ptr ? 0 : length(u)
    ns = s isa Ptr ? 0 : length(s)
    GC.@preserve u s check(ccall((:rsys_query_weights_set, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}, Int64, Ptr{Float32}, Int64),
        m.h, u, nu, s, ns))
end
# (n_users, n_sel) of the weights held for the next request, 0 = none of that kind
function query_weights_pending(m::Model)
    out = zeros(Int64, 2)
    GC.@preserve out check(ccall((:rsys_query_weights_pending, LIB), Int32, (Ptr{Cvoid}, Ptr{Int64}), m.h, out))
    (out[1], out[2])
end
# Q (D, n_queries); group 0-based per query or nothing; hist: one vector of (medium, matchedid, status) tuples per query in list order;
# sel: one vector of (medium, matchedid) tuples per group.  Returns (ids, scores, counts) as retrieve_topk does.
function retrieve_request(m::Model, medium::Integer, Q::Matrix{Float32}, k::Integer; group = nothing, n_groups::Integer = size(Q, 2),
                          hist = nothing, sel = nothing)
    g = group === nothing ? Ptr{Int32}(C_NULL) : Vector{Int32}(group)
    hoff = hist === nothing ? Ptr{Int64}(C_NULL) : Int64[0; cumsum(Int64[length(h) for h in hist])]
    hmed = hist === nothing ? Ptr{Int32}(C_NULL) : Int32[x[1] for h in hist for x in h]
    hid = hist === nothing ? Ptr{Int32}(C_NULL) : Int32[x[2] for h in hist for x in h]
    hst = hist === nothing ? Ptr{Int32}(C_NULL) : Int32[x[3] for h in hist for x in h]
    soff = sel === nothing ? Ptr{Int64}(C_NULL) : Int64[0; cumsum(Int64[length(a) for a in sel])]
    smed = sel === nothing ? Ptr{Int32}(C_NULL) : Int32[x[1] for a in sel for x in a]
    sid = sel === nothing ? Ptr{Int32}(C_NULL) : Int32[x[2] for a in sel for x in a]
    ids = Matrix{Int32}(undef, k, n_groups); scores = Matrix{Float32}(undef, k, n_groups); counts = Vector{Int32}(undef, n_groups)
    GC.@preserve Q g hoff hmed hid hst soff smed sid ids scores counts check(ccall((:rsys_retrieve_request, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float32}, Int64, Ptr{Int32}, Int32, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32},
         Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Float32}, Ptr{Int32}),
        m.h, medium, Q, size(Q, 2), g, n_groups, hoff, hmed, hid, hst, soff, smed, sid, k, ids, scores, counts))
    ids, scores, counts
end
# the ranks [start[g], start[g] + len[g]) (0-based, 1 <= len <= 1024) of each group's ordering and its exact admissible count
# (rsys_retrieve_window).  Q (D, n_queries) or nothing (no queries: states without users); a group may have no queries.  Returns
# (ids (1024, n_groups), scores (1024, n_groups), counts, totals).
function retrieve_window(m::Model, medium::Integer, Q, start, len; group = nothing, n_groups::Integer = length(start), hist = nothing,
                         sel = nothing)
    q = Q === nothing ? Ptr{Float32}(C_NULL) : Matrix{Float32}(Q)
    nq = Q === nothing ? 0 : size(q, 2)
    g = group === nothing ? Ptr{Int32}(C_NULL) : Vector{Int32}(group)
    hoff = hist === nothing ? Ptr{Int64}(C_NULL) : Int64[0; cumsum(Int64[length(h) for h in hist])]
    hmed = hist === nothing ? Ptr{Int32}(C_NULL) : Int32[x[1] for h in hist for x in h]
    hid = hist === nothing ? Ptr{Int32}(C_NULL) : Int32[x[2] for h in hist for x in h]
    hst = hist === nothing ? Ptr{Int32}(C_NULL) : Int32[x[3] for h in hist for x in h]
    soff = sel === nothing ? Ptr{Int64}(C_NULL) : Int64[0; cumsum(Int64[length(a) for a in sel])]
    smed = sel === nothing ? Ptr{Int32}(C_NULL) : Int32[x[1] for a in sel for x in a]
    sid = sel === nothing ? Ptr{Int32}(C_NULL) : Int32[x[2] for a in sel for x in a]
    ws = Vector{Int64}(start); wl = Vector{Int32}(len)
    (length(ws) == n_groups && length(wl) == n_groups) || error("retrieve_window: one start and one length per group")
    ids = Matrix{Int32}(undef, 1024, n_groups); scores = Matrix{Float32}(undef, 1024, n_groups)
    counts = Vector{Int32}(undef, n_groups); totals = Vector{Int32}(undef, n_groups)
    GC.@preserve q g hoff hmed hid hst soff smed sid ws wl ids scores counts totals check(ccall((:rsys_retrieve_window, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Float32}, Int64, Ptr{Int32}, Int32, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32},
         Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Ptr{Int32}, Ptr{Int32}),
        m.h, medium, q, nq, g, n_groups, hoff, hmed, hid, hst, soff, smed, sid, ws, wl, ids, scores, counts, totals))
    ids, scores, counts, totals
end
# a page per state without users (compute.jl:490-514 `/add_item`; rsys_render_items): per group medium, offset, limit, penalties (4 x ng);
# sel[g] = [(medium, id), ...] or nothing.  Returns (page ids per group, exact totals).
function render_items(m::Model, medium, offset, limit, penalties::Matrix{Float32}; sel = nothing)
    gm = Vector{Int32}(medium); ng = length(gm)
    off = Vector{Int64}(offset); lim = Vector{Int32}(limit)
    soff = sel === nothing ? Ptr{Int64}(C_NULL) : Int64[0; cumsum(Int64[length(s) for s in sel])]
    smed = sel === nothing ? Ptr{Int32}(C_NULL) : Int32[x[1] for s in sel for x in s]
    sid = sel === nothing ? Ptr{Int32}(C_NULL) : Int32[x[2] for s in sel for x in s]
    cap = sum(Int64.(lim))
    ids = Vector{Int32}(undef, max(cap, 1)); ioff = Vector{Int64}(undef, ng + 1); total = Vector{Int32}(undef, ng)
    GC.@preserve gm off lim penalties soff smed sid ids ioff total check(ccall((:rsys_render_items, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Float32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int64, Ptr{Int64},
         Ptr{Int32}),
        m.h, ng, gm, off, lim, penalties, soff, smed, sid, ids, cap, ioff, total))
    [ids[ioff[j]+1:ioff[j+1]] for j in 1:ng], total
end
# ranking and reranking of retrieved candidates (Inference/render.jl:335-435): "{m}.related" as a SparseMatrixCSC (V_m x V_m) or nothing
# to clear; it is held on the device beside the retrieval tables
function rank_related_set(m::Model, medium::Integer, A)
    A === nothing && return check(ccall((:rsys_rank_related_set, LIB), Int32, (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float32}),
                                        m.h, medium, 0, C_NULL, C_NULL, C_NULL))
    cp = Vector{Int64}(A.colptr .- 1); rv = Vector{Int32}(A.rowval .- 1); nz = Vector{Float32}(A.nzval)
    GC.@preserve cp rv nz check(ccall((:rsys_rank_related_set, LIB), Int32, (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float32}),
        m.h, medium, size(A, 2), cp, rv, nz))
end
# idxs: one Vector of 0-based candidate ids per group; partialk and penalties (decay, mmr, same_series, related) per group; Q (D, n_users)
# the users' "{m}.retrieval" embeddings, group 0-based per user, r_masked one Vector{Float32} per user (its group's candidates), hist as
# retrieve_request.  retrieval_coef / rating_coefs (c0, c1) / rating_mean: the registry's, or nothing.  r: given ranking scores (one Vector
# per group) instead of computing them.  Returns (ids per group in pick order, ranking score per group).
function rank_request(m::Model, medium::Integer, idxs, partialk, penalties, Q::Matrix{Float32}, group, r_masked; hist = nothing,
                      retrieval_coef = nothing, rating_coefs = nothing, rating_mean = 0f0, r = nothing, want_ids::Bool = true)
    ng = length(idxs)
    off = Int64[0; cumsum(Int64[length(c) for c in idxs])]
    cid = Int32[reduce(vcat, idxs; init = Int32[])...]
    pk = Vector{Int32}(partialk)
    pen = Float32[x for p in penalties for x in p]
    g = Vector{Int32}(group)
    rm = r_masked === nothing ? Ptr{Float32}(C_NULL) : Float32[reduce(vcat, r_masked; init = Float32[])...]
    nrm = r_masked === nothing ? 0 : length(rm)
    hoff = hist === nothing ? Ptr{Int64}(C_NULL) : Int64[0; cumsum(Int64[length(h) for h in hist])]
    hmed = hist === nothing ? Ptr{Int32}(C_NULL) : Int32[x[1] for h in hist for x in h]
    hid = hist === nothing ? Ptr{Int32}(C_NULL) : Int32[x[2] for h in hist for x in h]
    hst = hist === nothing ? Ptr{Int32}(C_NULL) : Int32[x[3] for h in hist for x in h]
    rc = retrieval_coef === nothing ? Ptr{Float32}(C_NULL) : Float32[retrieval_coef]
    kc = rating_coefs === nothing ? Ptr{Float32}(C_NULL) : Vector{Float32}(rating_coefs)
    rin = r === nothing ? Ptr{Float32}(C_NULL) : Float32[reduce(vcat, r; init = Float32[])...]
    ids = want_ids ? Vector{Int32}(undef, off[end]) : Ptr{Int32}(C_NULL)
    rout = Vector{Float32}(undef, off[end])
    GC.@preserve off cid pk pen Q g rm hoff hmed hid hst rc kc rin ids rout check(ccall((:rsys_rank_request, LIB), Int32,
        (Ptr{Cvoid}, Int32, Int32, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}, Int64, Ptr{Int32}, Ptr{Float32}, Int64,
         Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}, Float32, Ptr{Float32}, Ptr{Int32}, Ptr{Float32}),
        m.h, medium, ng, off, cid, pk, pen, Q, size(Q, 2), g, rm, nrm, hoff, hmed, hid, hst, rc, kc, rating_mean, rin, ids, rout))
    picked = want_ids ? [ids[off[j]+1:off[j]+min(pk[j], length(idxs[j]))] for j in 1:ng] : nothing
    picked, [rout[off[j]+1:off[j+1]] for j in 1:ng]
end
# compute.jl:512-531 + render.jl:437-474 in one device pipeline (rsys_render_request).  Per group: medium, offset, limit, penalties (4 x ng);
# per user: group (0-based), its row of `rows` (retrieval inference rows) with its query token `token`, its row of `prefix` (the history
# part of its ranking rows, `stride` columns) with `desc` (4 x nu: nh, userid, gender, source) and `ts`.  hist[u] = [(medium, id, status), ...],
# sel[g] = [(medium, id), ...] or nothing; slots = the 4 adapter-bank slots (0.retrieval, 0.ranking, 1.retrieval, 1.ranking) or nothing;
# coef_have (2) / coefs (4 x 2) the registry's coefficients or nothing.  The caller wraps this in GC.@preserve of the arrays `rows` and
# `prefix` point to.  Returns (page ids per group, totals).
function render_request(m::Model, medium, offset, limit, penalties::Matrix{Float32}, group, rows::RsysBatch, token, prefix::RsysBatch,
                        stride::Integer, desc::Matrix{Int32}, ts; slots = nothing, hist = nothing, sel = nothing, coef_have = nothing,
                        coefs = nothing)
    gm = Vector{Int32}(medium); ng = length(gm)
    off = Vector{Int64}(offset); lim = Vector{Int32}(limit)
    g = Vector{Int32}(group); nu = length(g)
    tok = Vector{Int32}(token); tsv = Vector{Float64}(ts)
    sl = slots === nothing ? Ptr{Int32}(C_NULL) : Vector{Int32}(slots)
    hoff = hist === nothing ? Ptr{Int64}(C_NULL) : Int64[0; cumsum(Int64[length(h) for h in hist])]
    hmed = hist === nothing ? Ptr{Int32}(C_NULL) : Int32[x[1] for h in hist for x in h]
    hid = hist === nothing ? Ptr{Int32}(C_NULL) : Int32[x[2] for h in hist for x in h]
    hst = hist === nothing ? Ptr{Int32}(C_NULL) : Int32[x[3] for h in hist for x in h]
    soff = sel === nothing ? Ptr{Int64}(C_NULL) : Int64[0; cumsum(Int64[length(s) for s in sel])]
    smed = sel === nothing ? Ptr{Int32}(C_NULL) : Int32[x[1] for s in sel for x in s]
    sid = sel === nothing ? Ptr{Int32}(C_NULL) : Int32[x[2] for s in sel for x in s]
    ch = coef_have === nothing ? Ptr{Int32}(C_NULL) : Vector{Int32}(coef_have)
    cf = coefs === nothing ? Ptr{Float32}(C_NULL) : Vector{Float32}(vec(coefs))
    cap = sum(Int64.(lim))
    ids = Vector{Int32}(undef, max(cap, 1)); ioff = Vector{Int64}(undef, ng + 1); total = Vector{Int32}(undef, ng)
    GC.@preserve gm off lim penalties g tok desc tsv sl hoff hmed hid hst soff smed sid ch cf ids ioff total check(ccall((:rsys_render_request, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Float32}, Int64, Ptr{Int32}, Ref{RsysBatch}, Ptr{Int32}, Ref{RsysBatch}, Int32,
         Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32},
         Ptr{Float32}, Ptr{Int32}, Int64, Ptr{Int64}, Ptr{Int32}),
        m.h, ng, gm, off, lim, penalties, nu, g, rows, tok, prefix, stride, desc, tsv, sl, hoff, hmed, hid, hst, soff, smed, sid, ch, cf, ids, cap,
        ioff, total))
    [ids[ioff[j]+1:ioff[j+1]] for j in 1:ng], total
end
# the same page with the ranking forward on full-length histories through the per-user K/V cache (rsys_render_request_full): no prefix;
# desc[1, u] = n_hist in 0:S-1, the history columns of row u of `rows`
function render_request_full(m::Model, medium, offset, limit, penalties::Matrix{Float32}, group, rows::RsysBatch, token, desc::Matrix{Int32},
                             ts; slots = nothing, hist = nothing, sel = nothing, coef_have = nothing, coefs = nothing)
    gm = Vector{Int32}(medium); ng = length(gm)
    off = Vector{Int64}(offset); lim = Vector{Int32}(limit)
    g = Vector{Int32}(group); nu = length(g)
    tok = Vector{Int32}(token); tsv = Vector{Float64}(ts)
    sl = slots === nothing ? Ptr{Int32}(C_NULL) : Vector{Int32}(slots)
    hoff = hist === nothing ? Ptr{Int64}(C_NULL) : Int64[0; cumsum(Int64[length(h) for h in hist])]
    hmed = hist === nothing ? Ptr{Int32}(C_NULL) : Int32[x[1] for h in hist for x in h]
    hid = hist === nothing ? Ptr{Int32}(C_NULL) : Int32[x[2] for h in hist for x in h]
    hst = hist === nothing ? Ptr{Int32}(C_NULL) : Int32[x[3] for h in hist for x in h]
    soff = sel === nothing ? Ptr{Int64}(C_NULL) : Int64[0; cumsum(Int64[length(s) for s in sel])]
    smed = sel === nothing ? Ptr{Int32}(C_NULL) : Int32[x[1] for s in sel for x in s]
    sid = sel === nothing ? Ptr{Int32}(C_NULL) : Int32[x[2] for s in sel for x in s]
    ch = coef_have === nothing ? Ptr{Int32}(C_NULL) : Vector{Int32}(coef_have)
    cf = coefs === nothing ? Ptr{Float32}(C_NULL) : Vector{Float32}(vec(coefs))
    cap = sum(Int64.(lim))
    ids = Vector{Int32}(undef, max(cap, 1)); ioff = Vector{Int64}(undef, ng + 1); total = Vector{Int32}(undef, ng)
    GC.@preserve gm off lim penalties g tok desc tsv sl hoff hmed hid hst soff smed sid ch cf ids ioff total check(ccall((:rsys_render_request_full, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Float32}, Int64, Ptr{Int32}, Ref{RsysBatch}, Ptr{Int32},
         Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32},
         Ptr{Float32}, Ptr{Int32}, Int64, Ptr{Int64}, Ptr{Int32}),
        m.h, ng, gm, off, lim, penalties, nu, g, rows, tok, desc, tsv, sl, hoff, hmed, hid, hst, soff, smed, sid, ch, cf, ids, cap,
        ioff, total))
    [ids[ioff[j]+1:ioff[j+1]] for j in 1:ng], total
end
function infer(m::Model, task::Integer, rows::Integer, S::Integer, D::Integer)   # model.py:531-538 over every token of the resident batch
    out = task == 0 ? Array{Float32}(undef, D, 2S, rows) : Array{Float32}(undef, 2S, rows)
    GC.@preserve out check(ccall((:rsys_infer, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Float32}, Int64), m.h, task, out, length(out))); out
end
function trunk_output(m::Model, rows::Integer, S::Integer, D::Integer)
    out = Array{Float32}(undef, D, 2S, rows)
    GC.@preserve out check(ccall((:rsys_trunk_output_get, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}, Int64), m.h, out, length(out))); out
end

# ---- optimizer state (checkpoint / resume, transformer.py:456-466,690-695)
function adamw_state(o::Optimizer, name::String, n::Integer)
    m = Vector{Float32}(undef, n); v = Vector{Float32}(undef, n); st = Ref{Int32}(0)
    GC.@preserve m v check(ccall((:rsys_adamw_state_get, LIB), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float32}, Ptr{Float32}, Int64, Ref{Int32}),
                                 o.h, name, m, v, n, st))
    (m, v, Int(st[]))
end
function adamw_state!(o::Optimizer, name::String, m::Vector{Float32}, v::Vector{Float32}, step::Integer)
    GC.@preserve m v check(ccall((:rsys_adamw_state_set, LIB), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float32}, Ptr{Float32}, Int64, Int32),
                                 o.h, name, m, v, length(m), step))
end

# ---- collectives beyond the gradient all-reduce
function allreduce_f64!(c::Comm, x::Vector{Float64})   # reduce_mean, transformer.py:199-204
    GC.@preserve x check(ccall((:rsys_allreduce_f64, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int32), c.h, x, length(x))); x
end
function grad_sync_early(m::Model)
    n = Ref{Int64}(0); check(ccall((:rsys_grad_sync_early, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}), m.h, n)); n[]
end
# the gradient reduction's bucket schedule of the last optimizer step: rows (first element, one past the last, phase)
function grad_sync_schedule(m::Model; cap::Integer = 64)
    out = zeros(Int64, 3 * cap); n = Ref{Int32}(0)
    GC.@preserve out check(ccall((:rsys_grad_sync_schedule, LIB), Int32, (Ptr{Cvoid}, Ptr{Int64}, Int32, Ref{Int32}), m.h, out, cap, n))
    permutedims(reshape(out[1:3 * min(Int(n[]), cap)], 3, :))
end
# (rank, world, transport, RCCL version code)
function comm_info(c::Comm)
    out = zeros(Int32, 4)
    GC.@preserve out check(ccall((:rsys_comm_info, LIB), Int32, (Ptr{Cvoid}, Ptr{Int32}), c.h, out)); out
end
# replica consistency (DDP's parameter broadcast, transformer.py:678-682, replaced by same-seed init + comparison): this rank's four
# checksum words travel in one slot per rank of a SUM all-reduce (the other slots zero: exact), then every rank compares all slots
function param_checksum(m::Model)
    out = zeros(Float64, 4)
    GC.@preserve out check(ccall((:rsys_param_checksum, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}), m.h, out)); out
end
function assert_replicas_equal(m::Model, c::Comm, rank::Integer, what::String = "")
    w = param_checksum(m); slots = zeros(Float64, 4 * c.world); slots[4rank + 1:4rank + 4] = w
    allreduce_f64!(c, slots)
    all(slots[4r + 1:4r + 4] == w for r in 0:c.world - 1) || error("replicas differ $what: $(reshape(slots, 4, :))")
end

# ---- instrumentation
step_mark!(m::Model) = check(ccall((:rsys_step_mark, LIB), Int32, (Ptr{Cvoid},), m.h))
function step_marks(m::Model, cap::Integer = 65536)
    ms = Vector{Float32}(undef, cap); n = Ref{Int32}(0)
    GC.@preserve ms check(ccall((:rsys_step_marks_get, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}, Int32, Ref{Int32}), m.h, ms, cap, n)); ms[1:n[]]
end
# RSYS_* environment switches (csrc/switches.hpp): parsed at model / communicator creation; reload_switches!() parses on demand
reload_switches!() = check(ccall((:rsys_switches_reload, LIB), Int32, ()))
function switches_set()
    buf = Vector{UInt8}(undef, 4096)
    GC.@preserve buf ccall((:rsys_switches_describe, LIB), Int32, (Ptr{UInt8}, Int32), buf, length(buf))
    unsafe_string(pointer(buf))
end
op_timing!(m::Model, mode::Integer) = check(ccall((:rsys_op_timing, LIB), Int32, (Ptr{Cvoid}, Int32), m.h, mode))
op_timing_filter!(m::Model, substr::AbstractString) = check(ccall((:rsys_op_timing_filter, LIB), Int32, (Ptr{Cvoid}, Cstring), m.h, substr))
function timing_report(m::Model)
    buf = Vector{UInt8}(undef, 1 << 16)
    GC.@preserve buf check(ccall((:rsys_timing_get, LIB), Int32, (Ptr{Cvoid}, Ptr{UInt8}, Csize_t), m.h, buf, length(buf)))
    unsafe_string(pointer(buf))
end

# Item-similarity LambdaRank model (Training/item_similarity/pairwise_ltr.py; DESIGN.md §4p): its own handle.  Arrays are 0-based ids,
# Julia column-major: features F x V, targets / relevance n x n_q, the export E x V.
mutable struct SimModel
    h::Ptr{Cvoid}
end
function SimModel(V::Integer, F::Integer, E::Integer; dtype = DTYPE_BF16, max_queries = 128, items_per_query = 2048, dropout = 0.1f0,
                  device = 0)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rsys_sim_create, LIB), Int32, (Int64, Int32, Int32, Int32, Int32, Int32, Float32, Int32, Ref{Ptr{Cvoid}}),
                V, F, E, dtype, max_queries, items_per_query, dropout, device, r))
    s = SimModel(r[])
    finalizer(x -> ccall((:rsys_sim_destroy, LIB), Int32, (Ptr{Cvoid},), x.h), s)
    s
end
sim_param_get(s::SimModel, name::AbstractString, out::Array{Float32}) =
    check(ccall((:rsys_sim_param_get, LIB), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float32}, Int64), s.h, name, out, length(out)))
sim_param_set!(s::SimModel, name::AbstractString, x::Array{Float32}) =
    check(ccall((:rsys_sim_param_set, LIB), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float32}, Int64), s.h, name, x, length(x)))
sim_grad_get(s::SimModel, name::AbstractString, out::Array{Float32}) =
    check(ccall((:rsys_sim_grad_get, LIB), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float32}, Int64), s.h, name, out, length(out)))
sim_zero_grad!(s::SimModel) = check(ccall((:rsys_sim_zero_grad, LIB), Int32, (Ptr{Cvoid},), s.h))
sim_features_set!(s::SimModel, f::Matrix{Float32}) =
    check(ccall((:rsys_sim_features_set, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64), s.h, f, size(f, 2), size(f, 1)))
# the rows of `medium` of a transformer model's item table, copied on the device (same device as the handle)
sim_features_from_model!(s::SimModel, m::Model, medium::Integer) =
    check(ccall((:rsys_sim_features_from_model, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32), s.h, m.h, medium))
function sim_forward_backward!(s::SimModel, source, target::Matrix{Int32}, relevance::Matrix{Float32}, weight; evaluate = false,
                               seed = 0, step = 0)
    src = Vector{Int32}(source); w = Vector{Float32}(weight); loss = Ref{Float32}(0)
    GC.@preserve src target relevance w check(ccall((:rsys_sim_forward_backward, LIB), Int32,
        (Ptr{Cvoid}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}, Int32, UInt64, UInt64, Ref{Float32}),
        s.h, length(src), size(target, 1), src, target, relevance, w, evaluate, seed, step, loss))
    loss[]
end
function sim_ndcg(s::SimModel, source, target::Matrix{Int32}, relevance::Matrix{Float32}, weight)
    src = Vector{Int32}(source); w = Vector{Float32}(weight); out = zeros(Float64, 2)
    GC.@preserve src target relevance w out check(ccall((:rsys_sim_ndcg, LIB), Int32,
        (Ptr{Cvoid}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float64}),
        s.h, length(src), size(target, 1), src, target, relevance, w, out))
    out[1], out[2]
end
function sim_adamw_step!(s::SimModel; lr = 3f-4, clip = 1f0)
    norm = Ref{Float32}(0); skipped = Ref{Int32}(0)
    check(ccall((:rsys_sim_adamw_step, LIB), Int32, (Ptr{Cvoid}, Float32, Float32, Ref{Float32}, Ref{Int32}), s.h, lr, clip, norm, skipped))
    norm[], skipped[] != 0
end
function sim_adamw_state_get(s::SimModel, name::AbstractString, n::Integer)
    m = zeros(Float32, n); v = zeros(Float32, n); step = Ref{Int32}(0)
    check(ccall((:rsys_sim_adamw_state_get, LIB), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float32}, Ptr{Float32}, Int64, Ref{Int32}),
                s.h, name, m, v, n, step))
    m, v, step[]
end
sim_embed_all!(s::SimModel, out::Matrix{Float32}; train_mode = false, seed = 0) =
    check(ccall((:rsys_sim_embed_all, LIB), Int32, (Ptr{Cvoid}, Int32, UInt64, Ptr{Float32}), s.h, train_mode, seed, out))
sim_export_set!(s::SimModel, emb::Matrix{Float32}) = check(ccall((:rsys_sim_export_set, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}), s.h, emb))
# bits: ceil(V / 32) x V Int32 words (column i = row i of the testmask)
sim_testmask_set!(s::SimModel, bits::Matrix{Int32}) = check(ccall((:rsys_sim_testmask_set, LIB), Int32, (Ptr{Cvoid}, Ptr{Int32}), s.h, bits))
# positives: one Vector{Int32} of 0-based ids per source; returns n x n_src ids in ascending score order
function sim_hard_negatives(s::SimModel, split::Integer, sources, positives, n::Integer)
    src = Vector{Int32}(sources)
    off = Int64[0; cumsum(Int64[length(p) for p in positives])]
    pid = Int32[reduce(vcat, positives; init = Int32[])...]
    out = Matrix{Int32}(undef, n, length(src))
    GC.@preserve src off pid out check(ccall((:rsys_sim_hard_negatives, LIB), Int32,
        (Ptr{Cvoid}, Int32, Int32, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Int32, Ptr{Int32}), s.h, split, length(src), src, off, pid, n, out))
    out
end
# pairwise_metrics.jl's ranking over the held export and testmask (DESIGN.md §4r): targets = one Vector of 0-based ids per source;
# returns the concatenated 1-based ranks among all items != source in sortperm(rev = true) order (0: target == source) and the offsets
function sim_pair_ranks(s::SimModel, sources, targets)
    src = Vector{Int32}(sources)
    off = Int64[0; cumsum(Int64[length(t) for t in targets])]
    tid = Int32[reduce(vcat, targets; init = Int32[])...]
    out = zeros(Int32, max(off[end], 1))
    GC.@preserve src off tid out check(ccall((:rsys_sim_pair_ranks, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}), s.h, length(src), src, off, tid, out))
    out[1:off[end]], off
end

# Search model (Training/search/train.py; DESIGN.md §4t): its own handle per medium.  Labels are 0-based medium-local ids; Julia
# column-major: features D x V_m, queries Q x B, "encoder.weight" D x Q, the export Q x V_m.
mutable struct SearchModel
    h::Ptr{Cvoid}
end
function SearchModel(V::Integer, D::Integer, Q::Integer; dtype = DTYPE_BF16, max_batch = 1024, device = 0)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rsys_search_create, LIB), Int32, (Int64, Int32, Int32, Int32, Int32, Int32, Ref{Ptr{Cvoid}}),
                V, D, Q, dtype, max_batch, device, r))
    s = SearchModel(r[])
    finalizer(x -> ccall((:rsys_search_destroy, LIB), Int32, (Ptr{Cvoid},), x.h), s)
    s
end
search_param_get(s::SearchModel, name::AbstractString, out::Array{Float32}) =
    check(ccall((:rsys_search_param_get, LIB), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float32}, Int64), s.h, name, out, length(out)))
search_param_set!(s::SearchModel, name::AbstractString, x::Array{Float32}) =
    check(ccall((:rsys_search_param_set, LIB), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float32}, Int64), s.h, name, x, length(x)))
search_grad_get(s::SearchModel, name::AbstractString, out::Array{Float32}) =
    check(ccall((:rsys_search_grad_get, LIB), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float32}, Int64), s.h, name, out, length(out)))
search_zero_grad!(s::SearchModel) = check(ccall((:rsys_search_zero_grad, LIB), Int32, (Ptr{Cvoid},), s.h))
search_features_set!(s::SearchModel, f::Matrix{Float32}) =
    check(ccall((:rsys_search_features_set, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64), s.h, f, size(f, 2), size(f, 1)))
search_features_from_model!(s::SearchModel, m::Model, medium::Integer) =
    check(ccall((:rsys_search_features_from_model, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32), s.h, m.h, medium))
# returns (loss, sum of the weights)
function search_forward_backward!(s::SearchModel, queries::Matrix{Float32}, labels, weight; evaluate = false)
    y = Vector{Int32}(labels); w = Vector{Float32}(weight); loss = Ref{Float32}(0); wsum = Ref{Float32}(0)
    GC.@preserve queries y w check(ccall((:rsys_search_forward_backward, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Int32}, Ptr{Float32}, Int32, Int32, Ref{Float32}, Ref{Float32}),
        s.h, queries, y, w, length(y), evaluate, loss, wsum))
    loss[], wsum[]
end
search_adamw_create!(s::SearchModel; beta1 = 0.9f0, beta2 = 0.999f0, eps = 1f-8, weight_decay = 0.1f0) =
    check(ccall((:rsys_search_adamw_create, LIB), Int32, (Ptr{Cvoid}, Float32, Float32, Float32, Float32), s.h, beta1, beta2, eps, weight_decay))
function search_adamw_step!(s::SearchModel; lr = 3f-4, clip = 1f0)
    norm = Ref{Float32}(0); skipped = Ref{Int32}(0)
    check(ccall((:rsys_search_adamw_step, LIB), Int32, (Ptr{Cvoid}, Float32, Float32, Ref{Float32}, Ref{Int32}), s.h, lr, clip, norm, skipped))
    norm[], skipped[] != 0
end
function search_adamw_state_get(s::SearchModel, name::AbstractString, n::Integer)
    m = zeros(Float32, n); v = zeros(Float32, n); step = Ref{Int32}(0)
    check(ccall((:rsys_search_adamw_state_get, LIB), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float32}, Ptr{Float32}, Int64, Ref{Int32}),
                s.h, name, m, v, n, step))
    m, v, step[]
end
search_adamw_state_set!(s::SearchModel, name::AbstractString, m::Array{Float32}, v::Array{Float32}, step::Integer) =
    check(ccall((:rsys_search_adamw_state_set, LIB), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float32}, Ptr{Float32}, Int64, Int32),
                s.h, name, m, v, length(m), step))
# "search.{m}": out is Q x V_m
search_export!(s::SearchModel, out::Matrix{Float32}) = check(ccall((:rsys_search_export, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}), s.h, out))
# queries Q x n; returns (0-based ids, log-probabilities), each k x n, best first, ties by ascending id
function search_topk(s::SearchModel, queries::Matrix{Float32}, k::Integer)
    n = size(queries, 2)
    ids = Matrix{Int32}(undef, k, n); lp = Matrix{Float32}(undef, k, n)
    GC.@preserve queries ids lp check(ccall((:rsys_search_topk, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}, Int32, Int32, Ptr{Int32}, Ptr{Float32}),
        s.h, queries, n, k, ids, lp))
    ids, lp
end
# text queries of the NEXT request call on the model (rsys_query_texts_set): x is Q x n_texts (embeddings of the search handle `s`, whose
# features are medium `medium`'s item table), group 0-based per text, w one finite Float32 per text or nothing (1.0 each).  An empty x
# clears the medium's set.  The six request calls that consume query weights consume both media's sets, on success and on error alike.
function query_texts_set(m::Model, s::SearchModel, medium::Integer, x::Matrix{Float32}, group, w = nothing)
    n = size(x, 2)
    g = Vector{Int32}(group)
    ww = w === nothing ? Ptr{Float32}(C_NULL) : Vector{Float32}(w)
    GC.@preserve x g ww check(ccall((:rsys_query_texts_set, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float32}, Int64, Ptr{Int32}, Ptr{Float32}), m.h, s.h, medium, x, n, g, ww))
end
# the texts held per medium for the next request, 0 = none
function query_texts_pending(m::Model)
    out = zeros(Int64, 2)
    GC.@preserve out check(ccall((:rsys_query_texts_pending, LIB), Int32, (Ptr{Cvoid}, Ptr{Int64}), m.h, out))
    (out[1], out[2])
end

# Watch-order counts (Training/media_relations.jl get_watch_order; DESIGN.md §4q): its own handle over the row band [row0, row1) of W.
# Ids are 0-based; W[a][b] = users who watched a before b.
mutable struct WatchOrder
    h::Ptr{Cvoid}
end
function WatchOrder(V::Integer; row0 = 0, row1 = V, device = 0)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rsys_watch_order_create, LIB), Int32, (Int64, Int64, Int64, Int32, Ref{Ptr{Cvoid}}), V, row0, row1, device, r))
    w = WatchOrder(r[])
    finalizer(x -> ccall((:rsys_watch_order_destroy, LIB), Int32, (Ptr{Cvoid},), x.h), w)
    w
end
# histories: one Vector{Int32} of 0-based ids per user (project_earliest's output)
function watch_order_add!(w::WatchOrder, histories)
    off = Int64[0; cumsum(Int64[length(h) for h in histories])]
    items = Int32[reduce(vcat, histories; init = Int32[])...]
    GC.@preserve off items check(ccall((:rsys_watch_order_add, LIB), Int32, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int32}),
                                       w.h, length(histories), off, items))
end
function watch_order_users(w::WatchOrder)
    n = Ref{Int64}(0)
    check(ccall((:rsys_watch_order_users, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}), w.h, n))
    n[]
end
# rows [row0, row0 + n_rows) as a V x n_rows matrix (column k = row row0 + k)
function watch_order_rows(w::WatchOrder, V::Integer, row0::Integer, n_rows::Integer)
    out = Matrix{Int32}(undef, V, n_rows)
    check(ccall((:rsys_watch_order_rows_get, LIB), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int32}), w.h, row0, n_rows, out))
    out
end
function watch_order_gather(w::WatchOrder, a::Vector{Int32}, b::Vector{Int32})
    out = Vector{Int32}(undef, length(a))
    check(ccall((:rsys_watch_order_gather, LIB), Int32, (Ptr{Cvoid}, Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}), w.h, length(a), a, b, out))
    out
end
# (indptr, indices, values) of the band, 0-based CSR
function watch_order_csr(w::WatchOrder, n_rows::Integer)
    nnz = Ref{Int64}(0)
    check(ccall((:rsys_watch_order_csr, LIB), Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Int64, Ref{Int64}),
                w.h, C_NULL, C_NULL, C_NULL, 0, nnz))
    indptr = Vector{Int64}(undef, n_rows + 1)
    indices = Vector{Int32}(undef, nnz[])
    values = Vector{Int32}(undef, nnz[])
    check(ccall((:rsys_watch_order_csr, LIB), Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Int64, Ref{Int64}),
                w.h, indptr, indices, values, nnz[], nnz))
    indptr, indices, values
end
watch_order_clear!(w::WatchOrder) = check(ccall((:rsys_watch_order_clear, LIB), Int32, (Ptr{Cvoid},), w.h))

# One optimizer step of train_epoch (transformer.py:256-276) with grad_accum = 1
function train_step!(m::Model, o::Optimizer, c::Union{Comm,Nothing}, task_w, lr_factor, seed, step)
    c === nothing || begin_grad_sync!(m, c)
    forward_backward!(m, false, task_w, 1f0, seed, step)
    c === nothing || allreduce_grads!(m, c)
    step!(o; lr_factor = Float32(lr_factor), clip = 1f0, grad_div = Float32(c === nothing ? 1 : c.world))
end

end # module
