# RRTXHip.jl -- Julia-side drop-in for the RRT^X extend/rewire hot path of
# jnetter6/RRTQX_3D, bound to librrtx_hip.so (include/rrtx.h) with ccall.
#
# Usage inside the reference (after its own includes, e.g. at the end of the
# include list of experimentsForRRTQX.jl):
#
#     include("DRRT_data_structures.jl"); include("jlist.jl"); ...   # unchanged reference files
#     include("/path/to/julia/RRTXHip.jl")
#     KD = HipTree{RRTNode{Float64}}(3)                 # instead of KDTree{RRTNode{Float64}}(d, KDdist)
#
# Every method below has the name, arity and return shape of the reference
# function it replaces, so extend()/findBestParent()/addNewObstacle() run
# unchanged on a HipTree.  NOTE: Julia is not installed in the build image, so
# this file has been written against Julia 1.0 semantics but not executed; the
# same C-ABI is exercised through ctypes by tests/ (rrtqx_3d_amd/_capi.py).

const LIBRRTX = get(ENV, "RRTX_HIP_LIB", "librrtx_hip.so")

const RRTX_OK = Cint(0)
const RRTX_E_CAPACITY = Cint(-2)
# RRTX_OPT_DUBINS_TIME_COLUMN and its values (include/rrtx.h): how the time column of a Dubins edge's trajectory is
# formed in a space with time -- the kernels' piecewise form (default) or the reference's running sum
const RRTX_OPT_DUBINS_TIME_COLUMN = Cint(16)
const RRTX_TIME_COLUMN_PIECEWISE = Int64(0)
const RRTX_TIME_COLUMN_RUNNING_SUM = Int64(1)

mutable struct HipTree{T}
  d::Int                       # fields the planner reads (R/rrtqx.jl:382, R/DRRT_Q.jl:2624,2631)
  treeSize::Int
  numWraps::Int
  root::T
  ctx::Ptr{Cvoid}
  nodes::Vector{T}             # device index (0-based) + 1 -> node; the reference has no node ids
  obsSig::UInt64               # signature of the obstacle list last uploaded
  indexOf::IdDict{Any,Int32}   # node -> 0-based device index (for edges given as node pairs)

  function HipTree{T}(d::Int; device::Int = 0, capacity::Int = 1 << 16) where {T}
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:rrtx_create, LIBRRTX), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Int64), ref, d, device, capacity)
    rc == RRTX_OK || error(unsafe_string(ccall((:rrtx_create_error, LIBRRTX), Cstring, ())))
    t = new{T}(d, 0, 0)
    t.ctx = ref[]
    t.nodes = Vector{T}()
    t.obsSig = UInt64(0)
    t.indexOf = IdDict{Any,Int32}()
    finalizer(x -> ccall((:rrtx_destroy, LIBRRTX), Cint, (Ptr{Cvoid},), x.ctx), t)
    return t
  end
end

# KDTree{T}(d, f, wraps, wrapPoints)  (R/kdTree_general.jl:108); wraps are 1-based dimensions
function HipTree{T}(d::Int, f::Function, wraps::Array{Int}, wrapPoints::Array{Float64}) where {T}
  t = HipTree{T}(d)
  for i = 1:length(wraps)
    rrtx_check(t, ccall((:rrtx_set_wrap, LIBRRTX), Cint, (Ptr{Cvoid}, Cint, Cdouble), t.ctx, wraps[i] - 1, wrapPoints[i]))
  end
  t.numWraps = length(wraps)
  return t
end
HipTree{T}(d::Int, f::Function) where {T} = HipTree{T}(d)

# non-zero status -> error(), the reference's only failure idiom (R/rrtqx.jl:70,91)
function rrtx_check(t::HipTree, rc::Cint)
  rc == RRTX_OK && return
  error(unsafe_string(ccall((:rrtx_last_error, LIBRRTX), Cstring, (Ptr{Cvoid},), t.ctx)))
end

# ---------------------------------------------------------------------------
# kdInsert (R/kdTree_general.jl:121-170)
function kdInsert(tree::HipTree{T}, node::T) where {T}
  if node.kdInTree
    return
  end
  node.kdInTree = true
  pos = vec(convert(Array{Float64}, node.position))          # 1 x d row -> d contiguous doubles
  first = Ref{Int64}(0)
  GC.@preserve pos rrtx_check(tree, ccall((:rrtx_nodes_append, LIBRRTX), Cint,
      (Ptr{Cvoid}, Ptr{Cdouble}, Int64, Ref{Int64}), tree.ctx, pos, 1, first))
  push!(tree.nodes, node)
  tree.indexOf[node] = Int32(first[])
  if tree.treeSize == 0
    tree.root = node
  end
  tree.treeSize += 1
end

# kdFindNearest (R/kdTree_general.jl:357-385) -> (node, dist)
function kdFindNearest(tree::HipTree{T}, queryPoint::Array{Float64}) where {T}
  q = vec(queryPoint)
  idx = Ref{Int32}(0); dist = Ref{Float64}(0.0)
  GC.@preserve q rrtx_check(tree, ccall((:rrtx_nn_nearest, LIBRRTX), Cint,
      (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ref{Int32}, Ref{Float64}), tree.ctx, q, 1, idx, dist))
  return (tree.nodes[idx[] + 1], dist[])
end

# kdFindNearestWithGuesstree (R/kdTree_general.jl:503-534): the guess only seeds the reference's descent
kdFindNearestWithGuesstree(tree::HipTree{T}, queryPoint::Array{Float64}, guess::T) where {T} =
  kdFindNearest(tree, queryPoint)

# kdFindKNearest (R/kdTree_general.jl:696-723) -> Array of nodes, node.data = distance.
# max(k, 2) nodes like the reference (its heap starts with root + dummy); ascending distance.
function kdFindKNearest(tree::HipTree{T}, k::Int, queryPoint::Array{Float64}) where {T}
  q = vec(queryPoint)
  w = max(k, 2)
  idx = Array{Int32}(undef, w); dist = Array{Float64}(undef, w); cnt = Ref{Int32}(0)
  GC.@preserve q idx dist rrtx_check(tree, ccall((:rrtx_nn_knearest, LIBRRTX), Cint,
      (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Ptr{Int32}, Ptr{Cdouble}, Ref{Int32}),
      tree.ctx, q, 1, k, idx, dist, cnt))
  ret = Array{T}(undef, cnt[], 1)
  for j = 1:cnt[]
    ret[j, 1] = tree.nodes[idx[j] + 1]
    ret[j, 1].data = dist[j]
  end
  return ret
end

# addToRangeList (R/kdTree_general.jl:765-771)
function addToRangeList(S::Tlist, thisNode::T, key::Float64) where {Tlist, T}
  if thisNode.inHeap
    return
  end
  thisNode.inHeap = true
  JlistPush(S, thisNode, key)
end

# kdFindMoreWithinRange (R/kdTree_general.jl:927-955): neighbours are appended to L with
# key = distance; membership and keys equal the reference's, list order is by node index.
function kdFindMoreWithinRange(tree::HipTree{T}, range::Float64, queryPoint::Array{Float64}, L::TL) where {T, TL}
  q = vec(queryPoint)
  r = [range]
  offsets = Vector{Int64}(undef, 2)
  cap = 256
  while true
    idx = Vector{Int32}(undef, cap); dist = Vector{Float64}(undef, cap)
    needed = Ref{Int64}(0)
    rc = GC.@preserve q r offsets idx dist ccall((:rrtx_nn_radius, LIBRRTX), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Ptr{Int64}, Ptr{Int32}, Ptr{Cdouble}, Int64, Ref{Int64}),
        tree.ctx, q, r, 0, 1, offsets, idx, dist, cap, needed)
    if rc == RRTX_E_CAPACITY            # two-call pattern: retry with the size the library reports
      cap = Int(needed[])
      continue
    end
    rrtx_check(tree, rc)
    for k = Int(needed[]):-1:1           # push in reverse so the list reads in ascending index order
      addToRangeList(L, tree.nodes[idx[k] + 1], dist[k])
    end
    return L
  end
end

# kdFindWithinRange (R/kdTree_general.jl:889-919)
function kdFindWithinRange(tree::HipTree{T}, range::Float64, queryPoint::Array{Float64}) where {T}
  L = JList{T}()
  return kdFindMoreWithinRange(tree, range, queryPoint, L)
end
# popFromRangeList / emptyRangeList (R/kdTree_general.jl:774-787) work on the JList unchanged.

# ---------------------------------------------------------------------------
# file dumps: the reference's writers recurse over kdChildL / kdChildR (R/DRRT_Q.jl:250-364), which a
# HipTree does not have; these walk tree.nodes in insertion order (same rows, different row order).
function saveRRTTree(tree::HipTree{T}, fileName) where {T}
  fptr = open(fileName, "w")
  for node in tree.nodes
    if node.rrtParentUsed
      writedlm(fptr, [node.position node.rrtTreeCost], ',')
      writedlm(fptr, [node.rrtParentEdge.endNode.position node.rrtParentEdge.endNode.rrtTreeCost], ',')
    end
  end
  close(fptr)
end

function saveRRTGraph(tree::HipTree{T}, fileName) where {T}          # R/DRRT_Q.jl:279-306
  fptr = open(fileName, "w")
  for node in tree.nodes
    listItem = node.rrtNeighborsOut.front
    for i = 1:node.rrtNeighborsOut.length
      writedlm(fptr, node.position, ',')
      writedlm(fptr, listItem.data.position, ',')
      listItem = listItem.child
    end
  end
  close(fptr)
end

function saveRRTNodes(tree::HipTree{T}, fileName) where {T}
  fptr = open(fileName, "w")
  for node in tree.nodes
    writedlm(fptr, [node.position node.rrtTreeCost node.rrtLMC], ',')
  end
  close(fptr)
end

function saveRRTNodesCollision(tree::HipTree{T}, fileName) where {T}
  fptr = open(fileName, "w")
  for node in tree.nodes
    writedlm(fptr, [node.position min(node.rrtTreeCost, node.rrtLMC)], ',')
  end
  close(fptr)
end

# ---------------------------------------------------------------------------
# obstacle list upload: CSpace.obstacles in list order (front first, R/list.jl:53-58)
function syncObstacles(tree::HipTree, S::TS) where {TS}
  m = S.obstacles.length
  cxyzr = Array{Float64}(undef, 4, m)       # column-major 4 x m == row-major m x 4 on the C side
  active = Vector{UInt8}(undef, m)
  sig = UInt64(m)
  ptr = S.obstacles.front
  for i = 1:m
    ob = ptr.data
    cxyzr[1:3, i] = ob.position[1:3]
    cxyzr[4, i] = ob.radius
    active[i] = (ob.obstacleUnused || ob.lifeSpan <= 0) ? 0x00 : 0x01   # R/DRRT_Q.jl:1777
    # (position included: the planner moves dynamic spheres in place, R/rrtqx.jl:453-584)
    sig = hash((objectid(ob), ob.position[1], ob.position[2], ob.position[3], ob.radius, active[i]), sig)
    ptr = ptr.child
  end
  # extend_candidates checks against the sphere list (RRTX_OPT_EXTEND_OBSTACLES = 8, value 0), whatever a
  # syncPolygonObstacles call in between has selected
  rrtx_check(tree, ccall((:rrtx_set_option, LIBRRTX), Cint, (Ptr{Cvoid}, Cint, Int64), tree.ctx, 8, 0))
  if sig != tree.obsSig
    GC.@preserve cxyzr active rrtx_check(tree, ccall((:rrtx_spheres_set, LIBRRTX), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{UInt8}, Cint), tree.ctx, cxyzr, active, m))
    tree.obsSig = sig
  end
end

# the same for List{Obstacle} (legacy 2-D / Dubins path): kinds 1, 3 and the moving kinds 6 / 7, whose
# Obstacle.path (rows dx, dy, t) goes up with rrtx_polygon_paths_set.  Call again whenever the host
# changed a path (changeObstacleDirection, R/DRRT.jl:370-443).  Edge / point checks then go through
# rrtx_edges_check / rrtx_points_check with kind = 1 and read time from the third coordinate.
function syncPolygonObstacles(tree::HipTree, S::TS) where {TS}
  # extend_candidates then checks against this list (RRTX_OPT_EXTEND_OBSTACLES = 8, value 1 = polygons)
  rrtx_check(tree, ccall((:rrtx_set_option, LIBRRTX), Cint, (Ptr{Cvoid}, Cint, Int64), tree.ctx, 8, 1))
  m = S.obstacles.length
  vertOff = zeros(Int32, m + 1); pathOff = zeros(Int32, m + 1)
  vxy = Float64[]; pxyt = Float64[]
  cr = Array{Float64}(undef, 3, m)
  kind = Vector{UInt8}(undef, m); active = Vector{UInt8}(undef, m)
  ptr = S.obstacles.front
  for i = 1:m
    ob = ptr.data
    moving = (ob.kind == 6 || ob.kind == 7)
    kind[i] = ob.kind
    active[i] = (ob.obstacleUnused || ob.lifeSpan <= 0) ? 0x00 : 0x01
    cr[1:2, i] = ob.position[1:2]; cr[3, i] = ob.radius
    poly = moving ? ob.originalPolygon : (ob.kind == 1 ? zeros(0, 2) : ob.polygon)
    for v = 1:size(poly, 1)
      push!(vxy, poly[v, 1], poly[v, 2])
    end
    vertOff[i + 1] = vertOff[i] + size(poly, 1)
    if moving
      for v = 1:size(ob.path, 1)
        push!(pxyt, ob.path[v, 1], ob.path[v, 2], ob.path[v, 3])
      end
    end
    pathOff[i + 1] = pathOff[i] + (moving ? size(ob.path, 1) : 0)
    ptr = ptr.child
  end
  GC.@preserve vertOff vxy cr kind active rrtx_check(tree, ccall((:rrtx_polygons_set, LIBRRTX), Cint,
      (Ptr{Cvoid}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt8}, Ptr{UInt8}, Cint),
      tree.ctx, vertOff, vxy, cr, kind, active, m))
  GC.@preserve pathOff pxyt rrtx_check(tree, ccall((:rrtx_polygon_paths_set, LIBRRTX), Cint,
      (Ptr{Cvoid}, Ptr{Int32}, Ptr{Cdouble}, Cint), tree.ctx, pathOff, pxyt, m))
end

# explicitEdgeCheck(C, edge) (R/DRRT_Q.jl:1802-1826) for SimpleEdge on sphere obstacles.
# The tree travels in a global per agent because the reference signature has no tree argument.
const HIP_TREE_OF = IdDict{Any, Any}()          # CSpace -> HipTree (set once per agent)
bindTree(S, tree::HipTree) = (HIP_TREE_OF[S] = tree)

function explicitEdgeCheckHip(S::TS, startPos::Array{Float64}, endPos::Array{Float64}, which::Int) where {TS}
  tree = HIP_TREE_OF[S]
  syncObstacles(tree, S)
  p0 = vec(startPos); p1 = vec(endPos)
  hit = Ref{UInt8}(0)
  GC.@preserve p0 p1 rrtx_check(tree, ccall((:rrtx_edges_check, LIBRRTX), Cint,
      (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Cint, Ref{UInt8}, Ptr{Int32}),
      tree.ctx, 0, p0, p1, 1, S.robotRadius, which, hit, C_NULL))
  return hit[] != 0x00
end

function explicitEdgeCheck(S::CSpace{T}, edge::SimpleEdge, verbose::Bool = false) where {T}
  if S.inWarmupTime                                # R/DRRT_Q.jl:1805-1807
    return false
  end
  return explicitEdgeCheckHip(S, edge.startNode.position, edge.endNode.position, -1)
end

# explicitEdgeCheck(S, edge, obstacle) (R/DRRT_SimpleEdge_functions.jl:210-212)
function explicitEdgeCheck(S::CSpace{T}, edge::SimpleEdge, obstacle::SphereObstacle) where {T}
  which = -1
  ptr = S.obstacles.front
  for i = 1:S.obstacles.length
    if ptr.data === obstacle
      which = i - 1
      break
    end
    ptr = ptr.child
  end
  which >= 0 || error("obstacle is not in CSpace.obstacles")
  return explicitEdgeCheckHip(S, edge.startNode.position, edge.endNode.position, which)
end

# explicitPointCheck (R/DRRT_Q.jl:1520-1556) -> (Bool, Float64)
function explicitPointCheck(S::CSpace{T}, point::Array{Float64}) where {T}
  if S.inWarmupTime
    return (false, Inf)
  end
  tree = HIP_TREE_OF[S]
  syncObstacles(tree, S)
  p = vec(point)
  unsafe = Ref{UInt8}(0); clr = Ref{Float64}(0.0)
  GC.@preserve p rrtx_check(tree, ccall((:rrtx_points_check, LIBRRTX), Cint,
      (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Int64, Cdouble, Cint, Ref{UInt8}, Ref{Float64}),
      tree.ctx, 0, p, 1, S.robotRadius, 1, unsafe, clr))
  return (unsafe[] != 0x00, clr[])
end

# explicitPointCheck3D (R/DRRT_Q.jl:1558-1590): the root check of the 3-D driver, no quick pass
function explicitPointCheck3D(S::CSpace{T}, point::Array{Float64}) where {T}
  if S.inWarmupTime
    return (false, Inf)
  end
  tree = HIP_TREE_OF[S]
  syncObstacles(tree, S)
  p = vec(point)
  unsafe = Ref{UInt8}(0); clr = Ref{Float64}(0.0)
  GC.@preserve p rrtx_check(tree, ccall((:rrtx_points_check, LIBRRTX), Cint,
      (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Int64, Cdouble, Cint, Ref{UInt8}, Ref{Float64}),
      tree.ctx, 0, p, 1, S.robotRadius, 0, unsafe, clr))
  return (unsafe[] != 0x00, clr[])
end

# explicitNodeCheck / explicitNodeCheck3D (R/DRRT_Q.jl:1594-1595)
explicitNodeCheck(S::CSpace{T}, node::RRTNode{T}) where {T} = explicitPointCheck(S, node.position)
explicitNodeCheck3D(S::CSpace{T}, node::RRTNode{T}) where {T} = explicitPointCheck3D(S, node.position)

# explicitPointCheck for a space whose obstacles are polygon Obstacles (R/DRRT.jl:1434-1470): call
# syncPolygonObstacles(tree, S) after every change of the list, then this
function explicitPointCheckPolygons(S::TS, point::Array{Float64}) where {TS}
  if S.inWarmupTime
    return (false, Inf)
  end
  tree = HIP_TREE_OF[S]
  p = vec(point)
  unsafe = Ref{UInt8}(0); clr = Ref{Float64}(0.0)
  GC.@preserve p rrtx_check(tree, ccall((:rrtx_points_check, LIBRRTX), Cint,
      (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Int64, Cdouble, Cint, Ref{UInt8}, Ref{Float64}),
      tree.ctx, 1, p, 1, S.robotRadius, 1, unsafe, clr))
  return (unsafe[] != 0x00, clr[])
end

# calculateTrajectory(S, ::SimpleEdge) (R/DRRT_SimpleEdge_functions.jl:177-181)
function calculateTrajectory(S::TS, edge::SimpleEdge) where {TS}
  tree = HIP_TREE_OF[S]
  s = vec(edge.startNode.position); g = vec(edge.endNode.position)
  d = Ref{Float64}(0.0); w = Ref{Float64}(0.0)
  GC.@preserve s g rrtx_check(tree, ccall((:rrtx_simple_steer, LIBRRTX), Cint,
      (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ref{Float64}, Ref{Float64}), tree.ctx, s, g, 1, d, w))
  edge.dist = d[]
  edge.distOriginal = edge.dist
  edge.Wdist = w[]
end

# ---------------------------------------------------------------------------
# Batched preamble of extend()/findBestParent (R/DRRT_Q.jl:1927-1979, 2546-2642): one call per
# batch of samples returns, per sample, the neighbour list with SimpleEdge costs and both directed
# collision flags, the nearest node and the sample's own point check.  findBestParent/extend then
# only do their list and heap bookkeeping.
struct ExtendCandidates
  offsets::Vector{Int64}      # nq + 1
  idx::Vector{Int32}          # 0-based node indices (tree.nodes[idx + 1])
  cost::Vector{Float64}       # edge.dist for both directions (SimpleEdge)
  hitOut::Vector{UInt8}       # explicitEdgeCheck(newNode -> near)
  hitIn::Vector{UInt8}        # explicitEdgeCheck(near -> newNode)
  nearestIdx::Vector{Int32}
  nearestDist::Vector{Float64}
  sampleUnsafe::Vector{UInt8}
end

function extend_candidates(tree::HipTree, S::TS, positions::Array{Float64,2}, hyberBallRad::Float64) where {TS}
  syncObstacles(tree, S)
  nq = size(positions, 2)                     # d x nq, each sample contiguous
  offsets = Vector{Int64}(undef, nq + 1)
  nidx = Vector{Int32}(undef, nq); ndist = Vector{Float64}(undef, nq); unsafe = Vector{UInt8}(undef, nq)
  cap = 64 * nq
  while true
    idx = Vector{Int32}(undef, cap); cost = Vector{Float64}(undef, cap)
    hout = Vector{UInt8}(undef, cap); hin = Vector{UInt8}(undef, cap)
    needed = Ref{Int64}(0)
    rc = GC.@preserve positions offsets idx cost hout hin nidx ndist unsafe ccall((:rrtx_extend_candidates, LIBRRTX), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cdouble, Cdouble, Ptr{Int64}, Ptr{Int32}, Ptr{Cdouble}, Ptr{UInt8}, Ptr{UInt8},
         Int64, Ref{Int64}, Ptr{Int32}, Ptr{Cdouble}, Ptr{UInt8}),
        tree.ctx, positions, nq, hyberBallRad, S.robotRadius, offsets, idx, cost, hout, hin, cap, needed, nidx, ndist, unsafe)
    if rc == RRTX_E_CAPACITY
      cap = Int(needed[])
      continue
    end
    rrtx_check(tree, rc)
    n = Int(needed[])
    return ExtendCandidates(offsets, idx[1:n], cost[1:n], hout[1:n], hin[1:n], nidx, ndist, unsafe)
  end
end

# The lists of extend_candidates are against the tree as it stood; this gives the lists of the batch's samples among
# themselves.  Row j: the batch positions i < j (0-based, ascending) with KDdist(q_j, q_i) < hyberBallRad -- what
# kdFindWithinRange adds to j's list when the samples are inserted one after the other -- with the SimpleEdge cost and
# the flags of q_j -> q_i (hitOut) and q_i -> q_j (hitIn).  skip: one byte per sample, non-zero = the sample has no
# list and is in none (sampleUnsafe of extend_candidates serves as it is).  The caller appends row j to the tree list of
# sample j with idx mapped to the node index each earlier sample received, dropping the samples it did not insert.
struct ExtendCandidatesSelf
  offsets::Vector{Int64}      # nq + 1
  idx::Vector{Int32}          # 0-based positions in the batch
  cost::Vector{Float64}
  hitOut::Vector{UInt8}
  hitIn::Vector{UInt8}
end

function extend_candidates_self(tree::HipTree, S::TS, positions::Array{Float64,2}, hyberBallRad::Float64;
                                skip::Union{Nothing,Vector{UInt8}} = nothing) where {TS}
  syncObstacles(tree, S)
  nq = size(positions, 2)                     # d x nq, each sample contiguous
  skip === nothing || length(skip) == nq || error("skip needs one byte per sample")
  skipArg = skip === nothing ? UInt8[] : skip
  skipPtr = skip === nothing ? Ptr{UInt8}(C_NULL) : pointer(skipArg)
  offsets = Vector{Int64}(undef, nq + 1)
  cap = max(8 * nq, 1024)
  while true
    idx = Vector{Int32}(undef, cap); cost = Vector{Float64}(undef, cap)
    hout = Vector{UInt8}(undef, cap); hin = Vector{UInt8}(undef, cap)
    needed = Ref{Int64}(0)
    rc = GC.@preserve positions skipArg offsets idx cost hout hin ccall((:rrtx_extend_candidates_self, LIBRRTX), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cdouble, Cdouble, Ptr{UInt8}, Ptr{Int64}, Ptr{Int32}, Ptr{Cdouble}, Ptr{UInt8},
         Ptr{UInt8}, Int64, Ref{Int64}),
        tree.ctx, positions, nq, hyberBallRad, S.robotRadius, skipPtr, offsets, idx, cost, hout, hin, cap, needed)
    if rc == RRTX_E_CAPACITY
      cap = Int(needed[])
      continue
    end
    rrtx_check(tree, rc)
    n = Int(needed[])
    return ExtendCandidatesSelf(offsets, idx[1:n], cost[1:n], hout[1:n], hin[1:n])
  end
end

# The closestNode rule of findBestParent (R/DRRT_Q.jl:1930-1935) for a batch: a sample whose ball is empty is linked to
# kdFindNearest over the tree as sequential insertion would have it, which may be an earlier sample of the same batch.
# Column j (k slots, Julia is column-major) holds the nearest live earlier batch positions i < j (0-based) ordered by
# (distance, i), with the SimpleEdge cost and the flags of q_j -> q_i (hitOut) and q_i -> q_j (hitIn) against the whole
# obstacle list; count[j] slots are used, the others have idx -1 and cost Inf.  skip: non-zero bytes take a sample out
# (sampleUnsafe of extend_candidates); want: the samples to fill (those whose tree list is empty; nothing: every live
# one); treeNearest: nearestIdx of extend_candidates, whose flags come back as treeHitOut / treeHitIn (empty otherwise).
# The caller walks column j, takes the first entry whose sample it inserted and links to it if its cost <
# nearestDist[j], else to the tree node; with count[j] == k, no inserted entry and the k-th cost below nearestDist[j]
# it searches the batch itself.
struct ExtendClosestSelf
  idx::Matrix{Int32}          # k x nq, 0-based positions in the batch, -1: unused
  cost::Matrix{Float64}
  hitOut::Matrix{UInt8}
  hitIn::Matrix{UInt8}
  count::Vector{Int32}
  treeHitOut::Vector{UInt8}
  treeHitIn::Vector{UInt8}
end

function extend_closest_self(tree::HipTree, S::TS, positions::Array{Float64,2}, k::Int;
                             skip::Union{Nothing,Vector{UInt8}} = nothing, want::Union{Nothing,Vector{UInt8}} = nothing,
                             treeNearest::Union{Nothing,Vector{Int32}} = nothing) where {TS}
  syncObstacles(tree, S)
  nq = size(positions, 2)                     # d x nq, each sample contiguous
  skip === nothing || length(skip) == nq || error("skip needs one byte per sample")
  want === nothing || length(want) == nq || error("want needs one byte per sample")
  treeNearest === nothing || length(treeNearest) == nq || error("treeNearest needs one index per sample")
  skipArg = skip === nothing ? UInt8[] : skip
  skipPtr = skip === nothing ? Ptr{UInt8}(C_NULL) : pointer(skipArg)
  wantArg = want === nothing ? UInt8[] : want
  wantPtr = want === nothing ? Ptr{UInt8}(C_NULL) : pointer(wantArg)
  nt = treeNearest === nothing ? 0 : nq
  treeArg = treeNearest === nothing ? Int32[] : treeNearest
  tho = Vector{UInt8}(undef, nt); thi = Vector{UInt8}(undef, nt)
  treePtr = treeNearest === nothing ? Ptr{Int32}(C_NULL) : pointer(treeArg)
  thoPtr = treeNearest === nothing ? Ptr{UInt8}(C_NULL) : pointer(tho)
  thiPtr = treeNearest === nothing ? Ptr{UInt8}(C_NULL) : pointer(thi)
  kk = max(k, 0)
  idx = Matrix{Int32}(undef, kk, nq); cost = Matrix{Float64}(undef, kk, nq)
  hout = Matrix{UInt8}(undef, kk, nq); hin = Matrix{UInt8}(undef, kk, nq)
  count = Vector{Int32}(undef, nq)
  rc = GC.@preserve positions skipArg wantArg treeArg idx cost hout hin count tho thi ccall((:rrtx_extend_closest_self, LIBRRTX), Cint,
      (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ptr{UInt8}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Ptr{Cdouble}, Ptr{UInt8},
       Ptr{UInt8}, Ptr{Int32}, Ptr{UInt8}, Ptr{UInt8}),
      tree.ctx, positions, nq, k, S.robotRadius, skipPtr, wantPtr, treePtr, idx, cost, hout, hin, count, thoPtr, thiPtr)
  rrtx_check(tree, rc)
  return ExtendClosestSelf(idx, cost, hout, hin, count, tho, thi)
end

# ---------------------------------------------------------------------------
# findBestParent (R/DRRT_Q.jl:1927-1979) and the rewire test of extend (:2619-2634) on the device, for a batch of
# samples: what comes back per sample is a status, a parent, the sample's rrtLMC and the neighbours to rewire -- the
# neighbour lists themselves stay on the device.  setNodeCosts uploads rrtLMC of the nodes a step changed
# (0-based first index; a node never set reads as Inf); extendSelect reads that array.  A sample with an empty ball
# (status RRTX_SEL_EMPTY) keeps the closestNode rule of findBestParent (:1931-1935) on the host: nearestIdx says which
# node.  The lists are against the tree as it stood (extend_candidates_self gives the samples' lists among themselves).
const RRTX_SEL_OK = UInt8(0)
const RRTX_SEL_NO_PARENT = UInt8(1)
const RRTX_SEL_EMPTY = UInt8(2)
const RRTX_SEL_UNSAFE = UInt8(3)
const RRTX_SEL_OVERFLOW = UInt8(4)

function setNodeCosts(tree::HipTree, firstIndex::Int, lmc::Vector{Float64})
  GC.@preserve lmc rrtx_check(tree, ccall((:rrtx_node_cost_set, LIBRRTX), Cint,
      (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Int64), tree.ctx, firstIndex, lmc, length(lmc)))
end

struct ExtendSelection
  status::Vector{UInt8}       # RRTX_SEL_*
  parentIdx::Vector{Int32}    # 0-based node index of the parent (-1 unless RRTX_SEL_OK)
  lmcNew::Vector{Float64}     # rrtLMC of the new node through that parent (Inf unless RRTX_SEL_OK)
  rwOffsets::Vector{Int64}    # nq + 1: the rewire candidates of sample i are rwOffsets[i] + 1 : rwOffsets[i + 1]
  rwNode::Vector{Int32}       # 0-based node index
  rwValue::Vector{Float64}    # the rrtLMC that node would get through the new node
  nearestIdx::Vector{Int32}
  nearestDist::Vector{Float64}
  sampleUnsafe::Vector{UInt8}
end

function extendSelect(tree::HipTree, S::TS, positions::Array{Float64,2}, hyberBallRad::Float64) where {TS}
  tree.d == 4 && return extend_select_dubins(tree, S, positions, hyberBallRad)   # [x y t theta]: DubinsEdge
  syncObstacles(tree, S)
  nq = size(positions, 2)                     # d x nq, each sample contiguous
  pidx = Vector{Int32}(undef, nq); pentry = Vector{Int64}(undef, nq); lmcNew = Vector{Float64}(undef, nq)
  status = Vector{UInt8}(undef, nq); rwoff = Vector{Int64}(undef, nq + 1)
  nidx = Vector{Int32}(undef, nq); ndist = Vector{Float64}(undef, nq); unsafe = Vector{UInt8}(undef, nq)
  rwcap = 16 * nq
  while true
    rwnode = Vector{Int32}(undef, rwcap); rwval = Vector{Float64}(undef, rwcap)
    rwneeded = Ref{Int64}(0); needed = Ref{Int64}(0)
    rc = GC.@preserve positions pidx pentry lmcNew status rwoff rwnode rwval nidx ndist unsafe ccall((:rrtx_extend_select, LIBRRTX), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int64}, Ptr{Cdouble}, Ptr{UInt8},
         Ptr{Int64}, Ptr{Int32}, Ptr{Cdouble}, Int64, Ref{Int64}, Ptr{Int32}, Ptr{Cdouble}, Ptr{UInt8}, Ptr{Int64},
         Ptr{Int32}, Ptr{Cdouble}, Ptr{UInt8}, Ptr{UInt8}, Int64, Ref{Int64}),
        tree.ctx, positions, nq, hyberBallRad, S.robotRadius, C_NULL, pidx, pentry, lmcNew, status, rwoff, rwnode, rwval,
        rwcap, rwneeded, nidx, ndist, unsafe, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, 0, needed)
    if rc == RRTX_E_CAPACITY
      rwcap = Int(rwneeded[])
      continue
    end
    rrtx_check(tree, rc)
    n = Int(rwneeded[])
    return ExtendSelection(status, pidx, lmcNew, rwoff, rwnode[1:n], rwval[1:n], nidx, ndist, unsafe)
  end
end

# device-pointer form over the lists rrtx_extend_candidates_dev / _dubins_dev left on the device (all arguments device
# pointers as Ptr{Cvoid}; for SimpleEdge lists pass the cost array as costOut and costIn; lmc = C_NULL: setNodeCosts' array)
function extendSelectDev(tree::HipTree, nq::Int, offsets, idx, costOut, costIn, hitOut, hitIn, nValid, cap::Int, unsafe, lmc,
                         parentIdx, parentEntry, lmcNew, status, rwOffsets, rwNode, rwValue, rwCap::Int, rwNeeded)
  rrtx_check(tree, ccall((:rrtx_extend_select_dev, LIBRRTX), Cint,
      (Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Int64}, Int64,
       Ptr{UInt8}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int64}, Ptr{Cdouble}, Ptr{UInt8}, Ptr{Int64}, Ptr{Int32}, Ptr{Cdouble},
       Int64, Ptr{Int64}),
      tree.ctx, nq, offsets, idx, costOut, costIn, hitOut, hitIn, nValid, cap, unsafe, lmc, parentIdx, parentEntry,
      lmcNew, status, rwOffsets, rwNode, rwValue, rwCap, rwNeeded))
end

# ---------------------------------------------------------------------------
# findNewTarget (R/DRRT_Q.jl:2901-2994) on the device: the search around the robot pose, the edge to every neighbour
# steered and checked, the neighbour with the lowest rrtLMC + edge.dist taken, the ball doubling while there is none.
# rrtLMC is read from the array setNodeCosts fills.  findNewTargets is the batch form (the agents of R/rrtqx.jl):
# poses is d x nq, r0 one first radius per pose; it returns the per-pose results without touching any RobotData.
const RRTX_TGT_OK = UInt8(0)
const RRTX_TGT_NOT_FOUND = UInt8(1)

struct NewTargets
  status::Vector{UInt8}       # RRTX_TGT_*
  targetIdx::Vector{Int32}    # 0-based node index (-1 unless RRTX_TGT_OK)
  edgeDist::Vector{Float64}   # edge.dist of pose -> target
  costToGoal::Vector{Float64} # rrtLMC(target) + edge.dist
  radiusUsed::Vector{Float64}
  rounds::Vector{Int32}
end

function findNewTargets(tree::HipTree, S::TS, poses::Array{Float64,2}, r0::Vector{Float64}, maxSearchBallRad::Float64) where {TS}
  nq = size(poses, 2)
  tidx = Vector{Int32}(undef, nq); edist = Vector{Float64}(undef, nq); cgoal = Vector{Float64}(undef, nq)
  rused = Vector{Float64}(undef, nq); rounds = Vector{Int32}(undef, nq); status = Vector{UInt8}(undef, nq)
  if tree.d == 4
    syncPolygonObstacles(tree, S)
    syncDubinsSpace(tree, S)
    GC.@preserve poses r0 tidx edist cgoal rused rounds status rrtx_check(tree, ccall((:rrtx_find_new_target_dubins, LIBRRTX), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble},
         Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{UInt8}),
        tree.ctx, poses, nq, r0, 1, maxSearchBallRad, S.robotRadius, S.minTurningRadius, C_NULL, tidx, edist, cgoal, rused,
        rounds, status))
  else
    syncObstacles(tree, S)
    GC.@preserve poses r0 tidx edist cgoal rused rounds status rrtx_check(tree, ccall((:rrtx_find_new_target, LIBRRTX), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble},
         Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{UInt8}),
        tree.ctx, poses, nq, r0, 1, maxSearchBallRad, S.robotRadius, C_NULL, tidx, edist, cgoal, rused, rounds, status))
  end
  return NewTargets(status, tidx, edist, cgoal, rused, rounds)
end

function findNewTarget(S::TS, KD::HipTree{T}, R::RobotData{T}, hyberBallRad::Float64) where {T, TS}
  R.robotEdgeUsed = false
  R.distAlongRobotEdge = 0.0
  R.timeAlongRobotEdge = 0.0
  R.robotEdgeForPlottingUsed = false
  R.distAlongRobotEdgeForPlotting = 0.0
  R.timeAlongRobotEdgeForPlotting = 0.0
  maxSearchBallRad = dist(S.lowerBounds, S.upperBounds)
  searchBallRad = min(max(hyberBallRad, dist(R.robotPose, R.nextMoveTarget.position)), maxSearchBallRad)
  out = findNewTargets(KD, S, reshape(copy(R.robotPose), KD.d, 1), [searchBallRad], maxSearchBallRad)
  if out.status[1] != RRTX_TGT_OK
    error("unable to find a valid move target")
  end
  R.nextMoveTarget = KD.nodes[out.targetIdx[1] + 1]
  R.distanceFromNextRobotPoseToNextMoveTarget = out.edgeDist[1]
  R.currentMoveInvalid = false
end

# ---------------------------------------------------------------------------
# addNewObstacle's edge loop (R/DRRT_Q.jl:3220-3290) against a device mirror of the planner's
# directed edges.  registerEdges is called where the planner creates edges (makeNeighborOf,
# makeInitialOutNeighborOf, makeParentOf); it returns the id of the first edge, ids are
# consecutive, the caller keeps `edges[id + 1]`.  obstacleSweep returns the 0-based ids of the
# registered edges that start within robotRadius + delta + ob.radius of `ob` and for which
# explicitEdgeCheck(S, edge, ob) is true; the caller sets their dist = Inf and updates its queues.
function registerEdges(tree::HipTree, edges::Vector{TE}) where {TE}
  n = length(edges)
  s = Int32[tree.indexOf[e.startNode] for e in edges]
  g = Int32[tree.indexOf[e.endNode] for e in edges]
  first = Ref{Int64}(0)
  GC.@preserve s g rrtx_check(tree, ccall((:rrtx_graph_edges_append, LIBRRTX), Cint,
      (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Int64, Ref{Int64}), tree.ctx, s, g, n, first))
  return Int(first[])
end

function obstacleSweep(tree::HipTree, S::TS, ob::SphereObstacle) where {TS}
  syncObstacles(tree, S)
  which = -1                                  # list position of ob (0-based)
  ptr = S.obstacles.front
  for i = 1:S.obstacles.length
    if ptr.data === ob
      which = i - 1
      break
    end
    ptr = ptr.child
  end
  which >= 0 || error("obstacle is not in CSpace.obstacles")
  cap = 4096
  while true
    ids = Vector{Int32}(undef, cap)
    needed = Ref{Int64}(0)
    rc = GC.@preserve ids ccall((:rrtx_obstacle_sweep, LIBRRTX), Cint,
        (Ptr{Cvoid}, Cint, Cdouble, Cdouble, Ptr{Int32}, Int64, Ref{Int64}),
        tree.ctx, which, S.robotRadius + S.delta + ob.radius, S.robotRadius, ids, cap, needed)
    if rc == RRTX_E_CAPACITY
      cap = Int(needed[])
      continue
    end
    rrtx_check(tree, rc)
    return ids[1:Int(needed[])]
  end
end

# The same for a burst of sphere obstacles -- the ones multirrtqx injects for the other agents in one iteration, or every
# obstacle re-added when the kino-distance grows -- in ONE pass over the registered edges (rrtx_obstacle_sweep_batch):
# one id vector per obstacle, in the order given, each exactly what obstacleSweep(tree, S, ob) returns.  block = true
# also sets dist = Inf for every returned edge in the device mirror (blockEdges over all of them, without the ids
# travelling back); the caller still sets edge.dist = Inf on its own edge objects.
function obstacleSweepBatch(tree::HipTree, S::TS, obs::Vector{SphereObstacle}, block::Bool = false) where {TS}
  syncObstacles(tree, S)
  k = length(obs)
  which = fill(Int32(-1), k)                  # list positions (0-based)
  ptr = S.obstacles.front
  for i = 1:S.obstacles.length
    for j = 1:k
      if ptr.data === obs[j]
        which[j] = i - 1
      end
    end
    ptr = ptr.child
  end
  all(which .>= 0) || error("obstacle is not in CSpace.obstacles")
  range = Float64[S.robotRadius + S.delta + ob.radius for ob in obs]
  offsets = Vector{Int64}(undef, k + 1)
  cap = 4096
  while true
    ids = Vector{Int32}(undef, cap)
    needed = Ref{Int64}(0)
    rc = GC.@preserve which range offsets ids ccall((:rrtx_obstacle_sweep_batch, LIBRRTX), Cint,
        (Ptr{Cvoid}, Ptr{Int32}, Cint, Ptr{Cdouble}, Cdouble, Cint, Ptr{Int64}, Ptr{Int32}, Int64, Ref{Int64}),
        tree.ctx, which, k, range, S.robotRadius, block ? 1 : 0, offsets, ids, cap, needed)
    if rc == RRTX_E_CAPACITY
      cap = Int(needed[])
      continue
    end
    rrtx_check(tree, rc)
    return [ids[Int(offsets[j]) + 1:Int(offsets[j + 1])] for j = 1:k]
  end
end

# The leaving half: the edge loops of removeObstacle (R/DRRT_Q.jl:3295-3362) for a burst of sphere obstacles that expire
# in one iteration, in ONE pass over the registered edges (rrtx_obstacle_release_batch) and as the loop is meant -- the
# reference marks ob unused first (:3302) and then frees nothing.  One id vector per obstacle, in the order given: the
# registered edges that are blocked, start within robotRadius + delta + ob.radius of ob, collide with it and with no
# obstacle that is in use and not in obs.  obstacleUnused of the obstacles in obs is not read.  unblock = true also
# sets dist = distOriginal for every returned edge in the device mirror (unblockEdges over all of them, without the ids
# travelling back); the caller still resets edge.dist on its own edge objects.
function obstacleReleaseBatch(tree::HipTree, S::TS, obs::Vector{SphereObstacle}, unblock::Bool = false) where {TS}
  syncObstacles(tree, S)
  k = length(obs)
  which = fill(Int32(-1), k)                  # list positions (0-based)
  ptr = S.obstacles.front
  for i = 1:S.obstacles.length
    for j = 1:k
      if ptr.data === obs[j]
        which[j] = i - 1
      end
    end
    ptr = ptr.child
  end
  all(which .>= 0) || error("obstacle is not in CSpace.obstacles")
  range = Float64[S.robotRadius + S.delta + ob.radius for ob in obs]
  offsets = Vector{Int64}(undef, k + 1)
  cap = 4096
  while true
    ids = Vector{Int32}(undef, cap)
    needed = Ref{Int64}(0)
    rc = GC.@preserve which range offsets ids ccall((:rrtx_obstacle_release_batch, LIBRRTX), Cint,
        (Ptr{Cvoid}, Ptr{Int32}, Cint, Ptr{Cdouble}, Cdouble, Cint, Ptr{Int64}, Ptr{Int32}, Int64, Ref{Int64}),
        tree.ctx, which, k, range, S.robotRadius, unblock ? 1 : 0, offsets, ids, cap, needed)
    if rc == RRTX_E_CAPACITY
      cap = Int(needed[])
      continue
    end
    rrtx_check(tree, rc)
    return [ids[Int(offsets[j]) + 1:Int(offsets[j + 1])] for j = 1:k]
  end
end

# The same for the POLYGON list (legacy planner, R/DRRT.jl:3048-3290; BASELINE config 5's discoverable / moving
# obstacles): findPointsInConflictWithObstacle(::Obstacle) -- Euclidean query, the Dubins one ([x y 0.0 pi], range +
# pi), one query per path segment for kinds 6 / 7 -- and the edge loop of addNewObstacle (remove = false) or
# removeObstacle (remove = true: blocked edges that collide with ob and with no other obstacle in use) in ONE call;
# the edge type is the tree's (d = 3 SimpleEdge, d = 4 DubinsEdge with S.minTurningRadius).
function obstacleSweep(tree::HipTree, S::TS, ob::Obstacle, remove::Bool = false) where {TS}
  syncPolygonObstacles(tree, S)
  which = -1
  ptr = S.obstacles.front
  for i = 1:S.obstacles.length
    if ptr.data === ob
      which = i - 1
      break
    end
    ptr = ptr.child
  end
  which >= 0 || error("obstacle is not in CSpace.obstacles")
  cap = 4096
  while true
    ids = Vector{Int32}(undef, cap)
    needed = Ref{Int64}(0)
    rc = GC.@preserve ids ccall((:rrtx_obstacle_sweep_polygon, LIBRRTX), Cint,
        (Ptr{Cvoid}, Cint, Cdouble, Cdouble, Cdouble, Cint, Ptr{Int32}, Int64, Ref{Int64}),
        tree.ctx, which, S.robotRadius, S.delta, S.minTurningRadius, remove ? 1 : 0, ids, cap, needed)
    if rc == RRTX_E_CAPACITY
      cap = Int(needed[])
      continue
    end
    rrtx_check(tree, rc)
    return ids[1:Int(needed[])]
  end
end

# The appearing half for a burst of POLYGON obstacles -- the ones a robot discovers in one main-loop iteration, each of
# which the reference hands to addNewObstacle (R/DRRT.jl:3127-3200) before one reduceInconsistency -- in ONE call
# (rrtx_obstacle_sweep_polygon_batch): one id vector per obstacle, in the order given, each exactly what
# obstacleSweep(tree, S, ob) returns.  block = true also sets dist = Inf for every returned edge in the device mirror
# (blockEdges over all of them, without the ids travelling back); the caller still sets edge.dist = Inf on its own edge
# objects.
function obstacleSweepBatch(tree::HipTree, S::TS, obs::Vector{Obstacle}, block::Bool = false) where {TS}
  syncPolygonObstacles(tree, S)
  k = length(obs)
  which = fill(Int32(-1), k)                  # list positions (0-based)
  ptr = S.obstacles.front
  for i = 1:S.obstacles.length
    for j = 1:k
      if ptr.data === obs[j]
        which[j] = i - 1
      end
    end
    ptr = ptr.child
  end
  all(which .>= 0) || error("obstacle is not in CSpace.obstacles")
  offsets = Vector{Int64}(undef, k + 1)
  cap = 4096
  while true
    ids = Vector{Int32}(undef, cap)
    needed = Ref{Int64}(0)
    rc = GC.@preserve which offsets ids ccall((:rrtx_obstacle_sweep_polygon_batch, LIBRRTX), Cint,
        (Ptr{Cvoid}, Ptr{Int32}, Cint, Cdouble, Cdouble, Cdouble, Cint, Ptr{Int64}, Ptr{Int32}, Int64, Ref{Int64}),
        tree.ctx, which, k, S.robotRadius, S.delta, S.minTurningRadius, block ? 1 : 0, offsets, ids, cap, needed)
    if rc == RRTX_E_CAPACITY
      cap = Int(needed[])
      continue
    end
    rrtx_check(tree, rc)
    return [ids[Int(offsets[j]) + 1:Int(offsets[j + 1])] for j = 1:k]
  end
end

# The leaving half for a burst of POLYGON obstacles -- the time-limited ones that expire in one main-loop iteration, each
# of which the reference hands to removeObstacle (R/DRRT.jl:3202-3290) before one reduceInconsistency -- in ONE call
# (rrtx_obstacle_release_polygon_batch), the burst taken as gone together: one id vector per obstacle, in the order
# given -- the registered edges that are blocked, start at a node in conflict with ob, collide with it and with no
# obstacle that is in use and not in obs; what obstacleSweep(tree, S, ob, true) returns with the others of obs marked
# unused.  ob itself must still be in use (the reference marks it unused after its loop, :3287): call setObstaclesUsed!
# afterwards.  unblock = true also sets dist = distOriginal for every returned edge in the device mirror (unblockEdges
# over all of them, without the ids travelling back); the caller still resets edge.dist on its own edge objects.
function obstacleReleaseBatch(tree::HipTree, S::TS, obs::Vector{Obstacle}, unblock::Bool = false) where {TS}
  syncPolygonObstacles(tree, S)
  k = length(obs)
  which = fill(Int32(-1), k)                  # list positions (0-based)
  ptr = S.obstacles.front
  for i = 1:S.obstacles.length
    for j = 1:k
      if ptr.data === obs[j]
        which[j] = i - 1
      end
    end
    ptr = ptr.child
  end
  all(which .>= 0) || error("obstacle is not in CSpace.obstacles")
  offsets = Vector{Int64}(undef, k + 1)
  cap = 4096
  while true
    ids = Vector{Int32}(undef, cap)
    needed = Ref{Int64}(0)
    rc = GC.@preserve which offsets ids ccall((:rrtx_obstacle_release_polygon_batch, LIBRRTX), Cint,
        (Ptr{Cvoid}, Ptr{Int32}, Cint, Cdouble, Cdouble, Cdouble, Cint, Ptr{Int64}, Ptr{Int32}, Int64, Ref{Int64}),
        tree.ctx, which, k, S.robotRadius, S.delta, S.minTurningRadius, unblock ? 1 : 0, offsets, ids, cap, needed)
    if rc == RRTX_E_CAPACITY
      cap = Int(needed[])
      continue
    end
    rrtx_check(tree, rc)
    return [ids[Int(offsets[j]) + 1:Int(offsets[j + 1])] for j = 1:k]
  end
end

# obstacleUnused = !used on the obstacles obs and, without sending the list again, on their places in the device list
# (rrtx_polygons_set_active): what removeObstacle does once its loop is over (R/DRRT.jl:3287), and what the discovery
# of an obstacle does before its sweep.  The list on the device must be the one of S (syncPolygonObstacles).
function setObstaclesUsed!(tree::HipTree, S::TS, obs::Vector{Obstacle}, used::Bool) where {TS}
  k = length(obs)
  which = fill(Int32(-1), k)                  # list positions (0-based)
  ptr = S.obstacles.front
  for i = 1:S.obstacles.length
    for j = 1:k
      if ptr.data === obs[j]
        which[j] = i - 1
      end
    end
    ptr = ptr.child
  end
  all(which .>= 0) || error("obstacle is not in CSpace.obstacles")
  for ob in obs
    ob.obstacleUnused = !used
  end
  active = fill(UInt8(used ? 1 : 0), k)
  GC.@preserve which active rrtx_check(tree, ccall((:rrtx_polygons_set_active, LIBRRTX), Cint,
      (Ptr{Cvoid}, Ptr{Int32}, Cint, Ptr{UInt8}), tree.ctx, which, k, active))
end

# edge.dist of registered edges first_id, first_id+1, ... (ids from registerEdges); registerEdges itself
# gives every edge the SimpleEdge cost of its two nodes.
function syncEdgeCosts(tree::HipTree, first_id::Int, edges::Vector{TE}) where {TE}
  d = Float64[e.dist for e in edges]
  GC.@preserve d rrtx_check(tree, ccall((:rrtx_graph_edges_set_dist, LIBRRTX), Cint,
      (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Int64), tree.ctx, first_id, d, length(d)))
end

# addNewObstacle's `edge.dist = Inf` (R/DRRT_Q.jl:3249) for the ids obstacleSweep returned
function blockEdges(tree::HipTree, ids::Vector{Int32})
  GC.@preserve ids rrtx_check(tree, ccall((:rrtx_graph_edges_block, LIBRRTX), Cint,
      (Ptr{Cvoid}, Ptr{Int32}, Int64), tree.ctx, ids, length(ids)))
end

# removeObstacle's `edge.dist = edge.distOriginal` (R/DRRT_Q.jl:3342) for the ids obstacleReleaseBatch returned
function unblockEdges(tree::HipTree, ids::Vector{Int32})
  GC.@preserve ids rrtx_check(tree, ccall((:rrtx_graph_edges_unblock, LIBRRTX), Cint,
      (Ptr{Cvoid}, Ptr{Int32}, Int64), tree.ctx, ids, length(ids)))
end

# cullCurrentNeighbors(node, hyberBallRad) (R/DRRT_Q.jl:2388-2403) over the registered edges, for the nodes given
# (nothing: every node of the tree): a node's current out-neighbour edges -- registered edges that start at it and end at
# a node inserted later -- whose edge.dist exceeds the ball are dropped (dist = distOriginal = Inf from then on, touched
# for the next costUpdateDelta); its initial ones stay.  Returns the number of edges dropped by this call.
function cullCurrentNeighbors(tree::HipTree, nodes, hyberBallRad::Float64)
  culled = Ref{Int64}(0)
  if nodes === nothing
    rrtx_check(tree, ccall((:rrtx_graph_edges_cull, LIBRRTX), Cint,
        (Ptr{Cvoid}, Cdouble, Ptr{Int32}, Int64, Ref{Int64}), tree.ctx, hyberBallRad, Ptr{Int32}(C_NULL), 0, culled))
  else
    which = Int32[tree.indexOf[nd] for nd in nodes]
    push!(which, Int32(0))                    # (an empty list is still a list: a pointer that is not NULL)
    GC.@preserve which rrtx_check(tree, ccall((:rrtx_graph_edges_cull, LIBRRTX), Cint,
        (Ptr{Cvoid}, Cdouble, Ptr{Int32}, Int64, Ref{Int64}), tree.ctx, hyberBallRad, which, length(which) - 1, culled))
  end
  return Int(culled[])
end

# Removes the edges cullCurrentNeighbors dropped; the others keep their order.  Returns (remap, edges removed):
# remap[old id + 1] = new id (0-based), -1 for a removed edge -- the caller renumbers the ids it holds with it; the
# device renumbers the parent edges and the baseline costUpdateDelta reports against.  Run costUpdateDelta between a cull
# and this: the device refuses (RRTX_E_STATE) while a dropped edge is still some node's parent edge.
function compactRegisteredEdges(tree::HipTree)
  ne = Int(ccall((:rrtx_graph_edges_count, LIBRRTX), Int64, (Ptr{Cvoid},), tree.ctx))
  remap = Vector{Int32}(undef, max(ne, 1))
  removed = Ref{Int64}(0)
  GC.@preserve remap rrtx_check(tree, ccall((:rrtx_graph_edges_compact, LIBRRTX), Cint,
      (Ptr{Cvoid}, Ptr{Int32}, Int64, Ref{Int64}), tree.ctx, remap, length(remap), removed))
  return remap[1:ne], Int(removed[])
end

# 1 for every registered edge of [firstId, firstId + n) that cullCurrentNeighbors dropped (registeredEdges cannot tell
# a dropped edge from one whose cost was set to Inf)
function culledEdges(tree::HipTree, firstId::Int, n::Int)
  out = Vector{UInt8}(undef, max(n, 1))
  GC.@preserve out rrtx_check(tree, ccall((:rrtx_graph_edges_get_culled, LIBRRTX), Cint,
      (Ptr{Cvoid}, Int64, Int64, Ptr{UInt8}), tree.ctx, firstId, n, out))
  return out[1:n]
end

# The state propogateDescendants + reduceInconsistency (R/DRRT_Q.jl:2703-2817) reach with changeThresh = 0.0
# once the queue is empty: rrtLMC of every node, and the registered id of its parent edge (-1: root / orphan).
# The caller writes them back: node.rrtLMC = node.rrtTreeCost = lmc[i+1]; makeParentOf along edge parent[i+1].
function costToRoot(tree::HipTree, root)
  n = length(tree.nodes)
  lmc = Vector{Float64}(undef, n)
  parent = Vector{Int32}(undef, n)
  passes = Ref{Int32}(0)
  GC.@preserve lmc parent rrtx_check(tree, ccall((:rrtx_graph_cost_to_root, LIBRRTX), Cint,
      (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Int32}, Ref{Int32}), tree.ctx, tree.indexOf[root], lmc, parent, passes))
  return lmc, parent
end

# costToRoot's update (rrtx_graph_cost_update) reported as the nodes it changed since the last call for this root:
# what propogateDescendants / reduceInconsistency (R/DRRT_Q.jl:2647-2817) touched.  Returns (node, lmc, parent):
# 0-based node indices (ascending), their rrtLMC (Inf: a new orphan), the registered id of their parent edge (-1: root /
# orphan).  store = true leaves rrtLMC of every node in the context's own device array (setNodeCosts' array).
function costUpdateDelta(tree::HipTree, root, store::Bool = false)
  cap = 4096
  while true
    node = Vector{Int32}(undef, cap)
    lmc = Vector{Float64}(undef, cap)
    parent = Vector{Int32}(undef, cap)
    needed = Ref{Int64}(0)
    passes = Ref{Int32}(0)
    rc = GC.@preserve node lmc parent ccall((:rrtx_graph_cost_update_delta, LIBRRTX), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Int32}, Ptr{Cdouble}, Ptr{Int32}, Int64, Ref{Int64}, Ref{Int32}),
        tree.ctx, tree.indexOf[root], store ? 1 : 0, node, lmc, parent, cap, needed, passes)
    if rc == RRTX_E_CAPACITY
      cap = Int(needed[])
      continue
    end
    rrtx_check(tree, rc)
    n = Int(needed[])
    return node[1:n], lmc[1:n], parent[1:n]
  end
end

# What extend() links for a batch (R/DRRT_Q.jl:2560-2640), registered on the device from the lists of
# extend_candidates* (0-based CSR as the calls return it): per inserted sample j (nodeOf[j] >= 0, its 0-based node index)
# and entry, the out-edge (dist = Inf when hitOut) and, when hitIn is clear, the in-edge -- in that order, ids consecutive
# from the count.  selfLists: idx holds 0-based batch positions (extend_candidates_self*); an entry whose sample was not
# inserted is dropped.  SimpleEdge lists pass the one cost array twice.  Returns (first id, edges registered, rowFirst):
# rowFirst[j] + 1 : rowFirst[j + 1] are the edges of sample j relative to the first id.
function registerEdgesFromLists(tree::HipTree, offsets::Vector{Int64}, idx::Vector{Int32}, costOut::Vector{Float64},
                                costIn::Vector{Float64}, hitOut::Vector{UInt8}, hitIn::Vector{UInt8},
                                nodeOf::Vector{Int32}, selfLists::Bool = false)
  nq = length(nodeOf)
  firstId = Ref{Int64}(0)
  added = Ref{Int64}(0)
  rowFirst = Vector{Int64}(undef, nq + 1)
  GC.@preserve offsets idx costOut costIn hitOut hitIn nodeOf rowFirst rrtx_check(tree,
    ccall((:rrtx_graph_edges_append_lists, LIBRRTX), Cint,
      (Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt8}, Ptr{UInt8}, Int64, Int64,
       Ptr{Int32}, Cint, Ref{Int64}, Ref{Int64}, Ptr{Int64}),
      tree.ctx, nq, offsets, idx, costOut, costIn, hitOut, hitIn, offsets[end], length(idx), nodeOf, selfLists ? 1 : 0,
      firstId, added, rowFirst))
  return Int(firstId[]), Int(added[]), rowFirst
end

# The same over lists that are already on the device (the *_dev extend calls): every array is a device pointer, nValid
# the count the extend call left there (C_NULL: not checked), rowFirst nq + 1 Int64 on the device or C_NULL.  Waits on
# the stream once, for the counts.
function registerEdgesFromListsDev(tree::HipTree, nq::Int, offsets::Ptr{Int64}, idx::Ptr{Int32}, costOut::Ptr{Cdouble},
                                   costIn::Ptr{Cdouble}, hitOut::Ptr{UInt8}, hitIn::Ptr{UInt8}, nValid::Ptr{Int64},
                                   cap::Int, nodeOf::Ptr{Int32}, selfLists::Bool = false,
                                   rowFirst::Ptr{Int64} = Ptr{Int64}(C_NULL))
  firstId = Ref{Int64}(0)
  added = Ref{Int64}(0)
  rrtx_check(tree, ccall((:rrtx_graph_edges_append_lists_dev, LIBRRTX), Cint,
      (Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Int64}, Int64,
       Ptr{Int32}, Cint, Ref{Int64}, Ref{Int64}, Ptr{Int64}),
      tree.ctx, nq, offsets, idx, costOut, costIn, hitOut, hitIn, nValid, cap, nodeOf, selfLists ? 1 : 0, firstId, added,
      rowFirst))
  return Int(firstId[]), Int(added[])
end

# The same over the lists the last extendSelect / extend_select_dubins left on the device: only nodeOf travels.  RRTX_E_STATE when another
# call has used the lists' workspaces since (kdInsert, setNodeCosts and the edge / cost calls keep them).
function registerSelectedEdges(tree::HipTree, nodeOf::Vector{Int32})
  nq = length(nodeOf)
  firstId = Ref{Int64}(0)
  added = Ref{Int64}(0)
  rowFirst = Vector{Int64}(undef, nq + 1)
  GC.@preserve nodeOf rowFirst rrtx_check(tree, ccall((:rrtx_graph_edges_append_selected, LIBRRTX), Cint,
      (Ptr{Cvoid}, Cint, Ptr{Int32}, Ref{Int64}, Ref{Int64}, Ptr{Int64}), tree.ctx, nq, nodeOf, firstId, added, rowFirst))
  return Int(firstId[]), Int(added[]), rowFirst
end

# (start, end, dist, distOriginal) of the registered edges ids (0-based ids, e.g. the parent edges costUpdateDelta names)
function registeredEdges(tree::HipTree, ids::Vector{Int32})
  n = length(ids)
  s = Vector{Int32}(undef, n)
  e = Vector{Int32}(undef, n)
  d = Vector{Float64}(undef, n)
  d0 = Vector{Float64}(undef, n)
  GC.@preserve ids s e d d0 rrtx_check(tree, ccall((:rrtx_graph_edges_get, LIBRRTX), Cint,
      (Ptr{Cvoid}, Ptr{Int32}, Int64, Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}), tree.ctx, ids, 0, n, s, e, d, d0))
  return s, e, d, d0
end


# ---------------------------------------------------------------------------
# Edge = DubinsEdge (R/DRRT_DubinsEdge.jl, R/DRRT_DubinsEdge_functions.jl; README's per-edge-type
# contract, R/README.txt:85-99).  The tree is a HipTree{RRTNode{Float64}}(4, KDdist, [4], [2pi]) and the
# obstacle list a List{Obstacle} (syncPolygonObstacles).  Call syncDubinsSpace(tree, S) once after the
# CSpace is configured (and again when spaceHasTime or the velocity bounds change).
function syncDubinsSpace(tree::HipTree, S::TS) where {TS}
  # RRTX_OPT_SPACE_HAS_TIME = 12: CSpace.spaceHasTime (R/DRRT_data_structures.jl:330)
  rrtx_check(tree, ccall((:rrtx_set_option, LIBRRTX), Cint, (Ptr{Cvoid}, Cint, Int64), tree.ctx, 12, S.spaceHasTime ? 1 : 0))
  rrtx_check(tree, ccall((:rrtx_set_dubins_velocity, LIBRRTX), Cint, (Ptr{Cvoid}, Cdouble, Cdouble),
      tree.ctx, S.dubinsMinVelocity, S.dubinsMaxVelocity))
end

# RRTX_TIME_COLUMN_RUNNING_SUM: every time stamp the Dubins entry points form or test is the reference's own running
# sum (R/DRRT_DubinsEdge_functions.jl:689-695), bit for bit; RRTX_TIME_COLUMN_PIECEWISE (default) the faster form.
function setDubinsTimeColumn(tree::HipTree, value::Integer)
  rrtx_check(tree, ccall((:rrtx_set_option, LIBRRTX), Cint, (Ptr{Cvoid}, Cint, Int64), tree.ctx,
      RRTX_OPT_DUBINS_TIME_COLUMN, Int64(value)))
end

# calculateTrajectory(S, ::DubinsEdge) (R/DRRT_DubinsEdge_functions.jl:329-709): dubinsType, Wdist, dist,
# distOriginal, velocity (space with time) and the discretised trajectory (P x 2, or P x 3 with time)
function calculateTrajectory(S::TS, edge::DubinsEdge) where {TS}
  tree = HIP_TREE_OF[S]
  s = vec(convert(Array{Float64}, edge.startNode.position)); g = vec(convert(Array{Float64}, edge.endNode.position))
  d = Ref{Float64}(0.0); w = Ref{Float64}(0.0); v = Ref{Float64}(0.0)
  word = Vector{UInt8}(undef, 3); ok = Ref{UInt8}(0)
  GC.@preserve s g word rrtx_check(tree, ccall((:rrtx_dubins_steer_full, LIBRRTX), Cint,
      (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Ref{Float64}, Ref{Float64}, Ref{Float64}, Ptr{UInt8}, Ref{UInt8}),
      tree.ctx, s, g, 1, S.minTurningRadius, d, w, v, word, ok))
  edge.dubinsType = String(copy(word))
  edge.Wdist = w[]
  edge.dist = d[]
  edge.distOriginal = edge.dist
  if S.spaceHasTime
    edge.velocity = v[]
  end
  if edge.Wdist == Inf                           # no trajectory is built (:661-662)
    return
  end
  # the row width is the CONTEXT's, not S's (the two can drift apart until syncDubinsSpace runs again); the call
  # refuses a width that is not the context's instead of overrunning `rows`
  hasTime = Ref{Int64}(0)
  rrtx_check(tree, ccall((:rrtx_get_option, LIBRRTX), Cint, (Ptr{Cvoid}, Cint, Ref{Int64}), tree.ctx, 12, hasTime))
  cols = hasTime[] != 0 ? 3 : 2
  off = Vector{Int64}(undef, 2)
  cap = 256
  while true
    rows = Array{Float64}(undef, cols, cap)      # column-major cols x cap == row-major cap x cols on the C side
    needed = Ref{Int64}(0)
    rc = GC.@preserve s g off rows ccall((:rrtx_dubins_trajectory, LIBRRTX), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Ptr{Int64}, Ptr{Cdouble}, Cint, Int64, Ref{Int64}),
        tree.ctx, s, g, 1, S.minTurningRadius, off, rows, cols, cap, needed)
    if rc == RRTX_E_CAPACITY
      cap = Int(needed[])
      continue
    end
    rrtx_check(tree, rc)
    edge.trajectory = copy(transpose(rows[:, 1:Int(needed[])]))
    return
  end
end

# validMove(S, ::DubinsEdge) (R/DRRT_DubinsEdge_functions.jl:115-125): host arithmetic on what
# calculateTrajectory stored, exactly the reference's expression
function validMove(S::TS, edge::DubinsEdge) where {TS}
  if S.spaceHasTime
    return ((edge.startNode.position[3] > edge.endNode.position[3]) && (S.dubinsMinVelocity <= edge.velocity <= S.dubinsMaxVelocity))
  end
  return true
end

# explicitEdgeCheck(C, edge) over the whole obstacle list (R/DRRT.jl:1660-1678 with the two-stage test of
# R/DRRT_DubinsEdge_functions.jl:750-774 per obstacle): one call steers and checks
function explicitEdgeCheck(S::CSpace{T}, edge::DubinsEdge, verbose::Bool = false) where {T}
  if S.inWarmupTime
    return false
  end
  tree = HIP_TREE_OF[S]
  s = vec(convert(Array{Float64}, edge.startNode.position)); g = vec(convert(Array{Float64}, edge.endNode.position))
  cost = Ref{Float64}(0.0); hit = Ref{UInt8}(0)
  GC.@preserve s g rrtx_check(tree, ccall((:rrtx_dubins_edges_check, LIBRRTX), Cint,
      (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Cdouble, Ref{Float64}, Ptr{UInt8}, Ref{UInt8}, Ptr{Int32}),
      tree.ctx, s, g, 1, S.minTurningRadius, S.robotRadius, cost, C_NULL, hit, C_NULL))
  return hit[] != 0x00
end

# explicitEdgeCheck(S, edge::DubinsEdge, obstacle) (R/DRRT_DubinsEdge_functions.jl:750-774) against ONE
# obstacle of the list: steering, the inflated chord test and every piece of the trajectory in one device call
# (round 2 composed it from two rrtx_edges_check launches per (edge, obstacle) on the host)
function explicitEdgeCheck(S::CSpace{T}, edge::DubinsEdge, obstacle::Obstacle) where {T}
  tree = HIP_TREE_OF[S]
  which = -1
  ptr = S.obstacles.front
  for i = 1:S.obstacles.length
    if ptr.data === obstacle
      which = i - 1
      break
    end
    ptr = ptr.child
  end
  which >= 0 || error("obstacle is not in CSpace.obstacles")
  s = vec(convert(Array{Float64}, edge.startNode.position)); g = vec(convert(Array{Float64}, edge.endNode.position))
  hit = Ref{UInt8}(0)
  GC.@preserve s g rrtx_check(tree, ccall((:rrtx_dubins_edges_check_obstacle, LIBRRTX), Cint,
      (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Cdouble, Cdouble, Cint, Ref{UInt8}),
      tree.ctx, s, g, 1, S.minTurningRadius, S.robotRadius, which, hit))
  return hit[] != 0x00
end

# Batched preamble of extend()/findBestParent for Edge = DubinsEdge (BASELINE configs 3 and 5): per sample
# the wrapped range search, both directed edges steered and checked; in a space with time a flag byte
# also carries bit 1 = !validMove, so `hit != 0` is findBestParent's whole blocking test (R/DRRT_Q.jl:1960).
struct ExtendCandidatesDubins
  offsets::Vector{Int64}
  idx::Vector{Int32}
  key::Vector{Float64}        # KDdist of the range search
  costOut::Vector{Float64}    # edge.dist newNode -> near
  costIn::Vector{Float64}     # edge.dist near -> newNode
  hitOut::Vector{UInt8}
  hitIn::Vector{UInt8}
  nearestIdx::Vector{Int32}
  nearestDist::Vector{Float64}
  sampleUnsafe::Vector{UInt8}
end

function extend_candidates_dubins(tree::HipTree, S::TS, positions::Array{Float64,2}, hyberBallRad::Float64) where {TS}
  nq = size(positions, 2)                     # 4 x nq
  offsets = Vector{Int64}(undef, nq + 1)
  nidx = Vector{Int32}(undef, nq); ndist = Vector{Float64}(undef, nq); unsafe = Vector{UInt8}(undef, nq)
  cap = 2048 * nq
  while true
    idx = Vector{Int32}(undef, cap); key = Vector{Float64}(undef, cap)
    cout = Vector{Float64}(undef, cap); cin = Vector{Float64}(undef, cap)
    hout = Vector{UInt8}(undef, cap); hin = Vector{UInt8}(undef, cap)
    needed = Ref{Int64}(0)
    rc = GC.@preserve positions offsets idx key cout cin hout hin nidx ndist unsafe ccall((:rrtx_extend_candidates_dubins, LIBRRTX), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cdouble, Cdouble, Cdouble, Ptr{Int64}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble},
         Ptr{Cdouble}, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Int64, Ref{Int64}, Ptr{Int32}, Ptr{Cdouble}, Ptr{UInt8}),
        tree.ctx, positions, nq, hyberBallRad, S.robotRadius, S.minTurningRadius, offsets, idx, key, cout, cin,
        C_NULL, C_NULL, hout, hin, cap, needed, nidx, ndist, unsafe)
    if rc == RRTX_E_CAPACITY
      cap = Int(needed[])
      continue
    end
    rrtx_check(tree, rc)
    n = Int(needed[])
    return ExtendCandidatesDubins(offsets, idx[1:n], key[1:n], cout[1:n], cin[1:n], hout[1:n], hin[1:n], nidx, ndist, unsafe)
  end
end

# extendSelect for a [x y t theta] tree: the lists of extend_candidates_dubins stay on the device, findBestParent and the
# rewire test run there over their two cost columns (costOut for the parent, costIn for the rewire test), and
# registerSelectedEdges then links them with both.  The polygon list and syncDubinsSpace are the caller's, as for
# extend_candidates_dubins.  nearestIdx is kdFindNearest in the wrapped space; asking for it does not cost the held lists.
function extend_select_dubins(tree::HipTree, S::TS, positions::Array{Float64,2}, hyberBallRad::Float64) where {TS}
  nq = size(positions, 2)                     # 4 x nq
  pidx = Vector{Int32}(undef, nq); pentry = Vector{Int64}(undef, nq); lmcNew = Vector{Float64}(undef, nq)
  status = Vector{UInt8}(undef, nq); rwoff = Vector{Int64}(undef, nq + 1)
  nidx = Vector{Int32}(undef, nq); ndist = Vector{Float64}(undef, nq); unsafe = Vector{UInt8}(undef, nq)
  rwcap = 16 * nq
  while true
    rwnode = Vector{Int32}(undef, rwcap); rwval = Vector{Float64}(undef, rwcap)
    rwneeded = Ref{Int64}(0); needed = Ref{Int64}(0)
    rc = GC.@preserve positions pidx pentry lmcNew status rwoff rwnode rwval nidx ndist unsafe ccall((:rrtx_extend_select_dubins, LIBRRTX), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int64}, Ptr{Cdouble},
         Ptr{UInt8}, Ptr{Int64}, Ptr{Int32}, Ptr{Cdouble}, Int64, Ref{Int64}, Ptr{Int32}, Ptr{Cdouble}, Ptr{UInt8},
         Ptr{Int64}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt8}, Ptr{UInt8}, Int64, Ref{Int64}),
        tree.ctx, positions, nq, hyberBallRad, S.robotRadius, S.minTurningRadius, C_NULL, pidx, pentry, lmcNew, status, rwoff,
        rwnode, rwval, rwcap, rwneeded, nidx, ndist, unsafe, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, 0, needed)
    if rc == RRTX_E_CAPACITY
      rwcap = Int(rwneeded[])
      continue
    end
    rrtx_check(tree, rc)
    n = Int(rwneeded[])
    return ExtendSelection(status, pidx, lmcNew, rwoff, rwnode[1:n], rwval[1:n], nidx, ndist, unsafe)
  end
end

# The lists of extend_candidates_dubins are against the tree as it stood; this gives the lists of the batch's samples
# among themselves, in the wrapped space.  Row j: the batch positions i < j (0-based, ascending) that kdFindWithinRange
# and its ghost iterator add to j's list when the samples are inserted one after the other, with the key of the first
# copy of q_j that reaches q_i and the Dubins cost and flags of q_j -> q_i (Out) and q_i -> q_j (In).  skip: one byte
# per sample, non-zero = the sample has no list and is in none (sampleUnsafe of extend_candidates_dubins serves as it
# is).  The caller appends row j to the tree list of sample j with idx mapped to the node index each earlier sample
# received, dropping the samples it did not insert.
struct ExtendCandidatesSelfDubins
  offsets::Vector{Int64}      # nq + 1
  idx::Vector{Int32}          # 0-based positions in the batch
  key::Vector{Float64}
  costOut::Vector{Float64}
  costIn::Vector{Float64}
  hitOut::Vector{UInt8}
  hitIn::Vector{UInt8}
end

function extend_candidates_self_dubins(tree::HipTree, S::TS, positions::Array{Float64,2}, hyberBallRad::Float64;
                                       skip::Union{Nothing,Vector{UInt8}} = nothing) where {TS}
  nq = size(positions, 2)                     # 4 x nq
  skip === nothing || length(skip) == nq || error("skip needs one byte per sample")
  skipArg = skip === nothing ? UInt8[] : skip
  skipPtr = skip === nothing ? Ptr{UInt8}(C_NULL) : pointer(skipArg)
  offsets = Vector{Int64}(undef, nq + 1)
  cap = max(8 * nq, 1024)
  while true
    idx = Vector{Int32}(undef, cap); key = Vector{Float64}(undef, cap)
    cout = Vector{Float64}(undef, cap); cin = Vector{Float64}(undef, cap)
    hout = Vector{UInt8}(undef, cap); hin = Vector{UInt8}(undef, cap)
    needed = Ref{Int64}(0)
    rc = GC.@preserve positions skipArg offsets idx key cout cin hout hin ccall((:rrtx_extend_candidates_self_dubins, LIBRRTX), Cint,
        (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cdouble, Cdouble, Cdouble, Ptr{UInt8}, Ptr{Int64}, Ptr{Int32}, Ptr{Cdouble},
         Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Int64, Ref{Int64}),
        tree.ctx, positions, nq, hyberBallRad, S.robotRadius, S.minTurningRadius, skipPtr, offsets, idx, key, cout, cin,
        C_NULL, C_NULL, hout, hin, cap, needed)
    if rc == RRTX_E_CAPACITY
      cap = Int(needed[])
      continue
    end
    rrtx_check(tree, rc)
    n = Int(needed[])
    return ExtendCandidatesSelfDubins(offsets, idx[1:n], key[1:n], cout[1:n], cin[1:n], hout[1:n], hin[1:n])
  end
end

# extend_closest_self for Edge = DubinsEdge: the closestNode rule of findBestParent (R/DRRT_Q.jl:1930-1935) in a Dubins
# batch.  Column j (k slots, Julia is column-major) holds the nearest live earlier batch positions i < j (0-based) in the
# wrapped space, ordered by (distance, i), the distance being the minimum over the copies of q_j; per slot the key and the
# Dubins cost and flags of q_j -> q_i (Out) and q_i -> q_j (In) against the whole polygon list; count[j] slots are used,
# the others have idx -1 and key / cost Inf.  skip: non-zero bytes take a sample out (sampleUnsafe of
# extend_candidates_dubins); want: the samples to fill (those whose tree list is empty; nothing: every live one);
# treeNearest: nearestIdx of extend_candidates_dubins, whose costs and flags come back in the tree* fields (empty
# otherwise).  The caller walks column j, takes the first entry whose sample it inserted and links to it if its key <
# nearestDist[j], else to the tree node; with count[j] == k, no inserted entry and the k-th key below nearestDist[j] it
# searches the batch itself.
struct ExtendClosestSelfDubins
  idx::Matrix{Int32}          # k x nq, 0-based positions in the batch, -1: unused
  key::Matrix{Float64}
  costOut::Matrix{Float64}
  costIn::Matrix{Float64}
  hitOut::Matrix{UInt8}
  hitIn::Matrix{UInt8}
  count::Vector{Int32}
  treeCostOut::Vector{Float64}
  treeCostIn::Vector{Float64}
  treeHitOut::Vector{UInt8}
  treeHitIn::Vector{UInt8}
end

function extend_closest_self_dubins(tree::HipTree, S::TS, positions::Array{Float64,2}, k::Int;
                                    skip::Union{Nothing,Vector{UInt8}} = nothing,
                                    want::Union{Nothing,Vector{UInt8}} = nothing,
                                    treeNearest::Union{Nothing,Vector{Int32}} = nothing) where {TS}
  nq = size(positions, 2)                     # 4 x nq
  skip === nothing || length(skip) == nq || error("skip needs one byte per sample")
  want === nothing || length(want) == nq || error("want needs one byte per sample")
  treeNearest === nothing || length(treeNearest) == nq || error("treeNearest needs one index per sample")
  skipArg = skip === nothing ? UInt8[] : skip
  skipPtr = skip === nothing ? Ptr{UInt8}(C_NULL) : pointer(skipArg)
  wantArg = want === nothing ? UInt8[] : want
  wantPtr = want === nothing ? Ptr{UInt8}(C_NULL) : pointer(wantArg)
  nt = treeNearest === nothing ? 0 : nq
  treeArg = treeNearest === nothing ? Int32[] : treeNearest
  tco = Vector{Float64}(undef, nt); tci = Vector{Float64}(undef, nt)
  tho = Vector{UInt8}(undef, nt); thi = Vector{UInt8}(undef, nt)
  treePtr = treeNearest === nothing ? Ptr{Int32}(C_NULL) : pointer(treeArg)
  tcoPtr = treeNearest === nothing ? Ptr{Cdouble}(C_NULL) : pointer(tco)
  tciPtr = treeNearest === nothing ? Ptr{Cdouble}(C_NULL) : pointer(tci)
  thoPtr = treeNearest === nothing ? Ptr{UInt8}(C_NULL) : pointer(tho)
  thiPtr = treeNearest === nothing ? Ptr{UInt8}(C_NULL) : pointer(thi)
  kk = max(k, 0)
  idx = Matrix{Int32}(undef, kk, nq); key = Matrix{Float64}(undef, kk, nq)
  cout = Matrix{Float64}(undef, kk, nq); cin = Matrix{Float64}(undef, kk, nq)
  hout = Matrix{UInt8}(undef, kk, nq); hin = Matrix{UInt8}(undef, kk, nq)
  count = Vector{Int32}(undef, nq)
  rc = GC.@preserve positions skipArg wantArg treeArg idx key cout cin hout hin count tco tci tho thi ccall((:rrtx_extend_closest_self_dubins, LIBRRTX), Cint,
      (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Cdouble, Cdouble, Ptr{UInt8}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Ptr{Cdouble},
       Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble},
       Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt8}),
      tree.ctx, positions, nq, k, S.robotRadius, S.minTurningRadius, skipPtr, wantPtr, treePtr, idx, key, cout, cin,
      C_NULL, C_NULL, hout, hin, count, tcoPtr, tciPtr, C_NULL, C_NULL, thoPtr, thiPtr)
  rrtx_check(tree, rc)
  return ExtendClosestSelfDubins(idx, key, cout, cin, hout, hin, count, tco, tci, tho, thi)
end
