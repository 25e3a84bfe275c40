### Additive R entry points over the batch routines of libpeaksegdisk_hip.so.  The five
### entry points of the package (PeakSegFPOP_file/_dir/_df/_vec, sequentialSearch_dir) keep
### working unchanged through .C("PeakSegFPOP_interface"); these are optional faster forms.

set_devices_knob <- function
### PEAKSEG_HIP_DEVICES for one call: NULL leaves the environment alone; "all" or device ids
### (e.g. 0:7) spread the call over those GPUs.  Returns what restore_devices_knob needs.
(devices){
  if(is.null(devices))return(NULL)
  old <- Sys.getenv("PEAKSEG_HIP_DEVICES", unset=NA)
  Sys.setenv(PEAKSEG_HIP_DEVICES=paste(devices, collapse=","))
  list(old=old)
}

restore_devices_knob <- function(saved){
  if(is.null(saved))return(invisible())
  if(is.na(saved$old)){
    Sys.unsetenv("PEAKSEG_HIP_DEVICES")
  }else{
    Sys.setenv(PEAKSEG_HIP_DEVICES=saved$old)
  }
  invisible()
}

PeakSegFPOP_dir_batch <- function
### PeakSegFPOP_dir for many (problem.dir, penalty) pairs: cached results are reused, the rest
### is solved in one launch (one parse and upload per coverage.bedGraph).  devices: "all" or
### GPU ids, one problem set per listed GPU, solved side by side.
(problem.dir.vec, penalty.vec, devices=NULL){
  stopifnot(is.character(problem.dir.vec), length(problem.dir.vec)==length(penalty.vec))
  n <- length(problem.dir.vec)
  saved <- set_devices_knob(devices)
  on.exit(restore_devices_knob(saved), add=TRUE)
  res <- .C(
    "PeakSegFPOP_dir_batch_interface",
    as.character(problem.dir.vec), paste(penalty.vec), as.integer(n),
    status=integer(n), cached=integer(n),
    PACKAGE="PeakSegDisk")
  if(any(res$status != 0)){
    stop("error code ", res$status[res$status != 0][1])
  }
  ## every pair now has consistent result files: these calls are cache hits
  mapply(PeakSegFPOP_dir, problem.dir.vec, paste(penalty.vec), SIMPLIFY=FALSE)
}

sequentialSearch_dir_resident <- function
### sequentialSearch_dir with the coverage parsed and uploaded once and the arena reused
### between penalties; same penalties, same files, same result as sequentialSearch_dir.
(problem.dir, peaks.int, verbose=0){
  stopifnot(is.integer(peaks.int) && length(peaks.int)==1 && 0 <= peaks.int)
  stopifnot(is.character(problem.dir) && length(problem.dir)==1)
  capacity <- 256L
  res <- .C(
    "PeakSegFPOP_search_interface",
    problem.dir, peaks.int, as.integer(verbose), capacity,
    penalty=rep(strrep(" ", 39), capacity), iteration=integer(capacity),
    under=integer(capacity), over=integer(capacity),
    n=integer(1), chosen=integer(1),
    PACKAGE="PeakSegDisk")
  i.vec <- seq_len(res$n)
  model.list <- lapply(i.vec, function(i){
    L <- PeakSegFPOP_dir(problem.dir, res$penalty[i])
    L$loss$iteration <- res$iteration[i]
    L$loss$under <- res$under[i]
    L$loss$over <- res$over[i]
    L
  })
  out <- model.list[[res$chosen]]
  out$others <- do.call(rbind, lapply(model.list, "[[", "loss"))[order(iteration)]
  out
}

sequentialSearch_dir_batch <- function
### sequentialSearch_dir on several problem directories at once: every directory gets the
### result sequentialSearch_dir(problem.dir, peaks.int) gives, but the models the searches ask
### for in the same iteration are computed in one launch on the GPU.  devices: "all" or GPU
### ids, the directories dealt to one shard per listed GPU.
(problem.dir.vec, peaks.int.vec, verbose=0, devices=NULL){
  stopifnot(is.character(problem.dir.vec), is.integer(peaks.int.vec), all(0 <= peaks.int.vec))
  n <- length(problem.dir.vec)
  saved <- set_devices_knob(devices)
  on.exit(restore_devices_knob(saved), add=TRUE)
  peaks.int.vec <- rep(peaks.int.vec, l=n)
  capacity <- 256L
  res <- .C(
    "PeakSegFPOP_search_batch_interface",
    problem.dir.vec, as.integer(n), peaks.int.vec, as.integer(verbose), capacity,
    penalty=rep(strrep(" ", 39), capacity*n), iteration=integer(capacity*n),
    under=integer(capacity*n), over=integer(capacity*n),
    n.models=integer(n), chosen=integer(n), status=integer(n),
    PACKAGE="PeakSegDisk")
  if(any(res$status != 0)){
    stop("error code ", res$status[res$status != 0][1])
  }
  lapply(seq_len(n), function(d){
    i.vec <- (d-1L)*capacity + seq_len(res$n.models[d])
    model.list <- lapply(i.vec, function(i){
      L <- PeakSegFPOP_dir(problem.dir.vec[d], res$penalty[i])
      L$loss$iteration <- res$iteration[i]
      L$loss$under <- res$under[i]
      L$loss$over <- res$over[i]
      L
    })
    out <- model.list[[res$chosen[d]]]
    out$others <- do.call(rbind, lapply(model.list, "[[", "loss"))[order(iteration)]
    out
  })
}

search_models <- function
### the value of a penalty search from the rows a native search returned: the chosen model with
### $others, every model read back with PeakSegFPOP_dir (cache hits)
(problem.dir, penalty, iteration, under, over, chosen){
  model.list <- lapply(seq_along(penalty), function(i){
    L <- PeakSegFPOP_dir(problem.dir, penalty[i])
    L$loss$iteration <- iteration[i]
    L$loss$under <- under[i]
    L$loss$over <- over[i]
    L
  })
  out <- model.list[[chosen]]
  out$others <- do.call(rbind, lapply(model.list, "[[", "loss"))[order(iteration)]
  out
}

parallelSearch_dir <- function
### The model with peaks.int peaks (or the next simpler one, as sequentialSearch_dir) found with
### width models per round instead of one: each round asks for the secant penalty of
### sequentialSearch_dir and up to width-1 more inside the bracket, all solved in one launch.
### width=0L: the library's default; width=1L: the penalties of sequentialSearch_dir.  devices:
### "all" or GPU ids, each round's models dealt over the listed GPUs.
(problem.dir, peaks.int, width=0L, verbose=0, devices=NULL){
  stopifnot(is.integer(peaks.int) && length(peaks.int)==1 && 0 <= peaks.int)
  stopifnot(is.character(problem.dir) && length(problem.dir)==1)
  stopifnot(is.integer(width) && length(width)==1 && 0 <= width && width <= 256)
  saved <- set_devices_knob(devices)
  on.exit(restore_devices_knob(saved), add=TRUE)
  capacity <- 1024L
  res <- .C(
    "PeakSegFPOP_parallel_search_interface",
    problem.dir, peaks.int, width, as.integer(verbose), capacity,
    penalty=rep(strrep(" ", 39), capacity), iteration=integer(capacity),
    under=integer(capacity), over=integer(capacity),
    n=integer(1), chosen=integer(1),
    PACKAGE="PeakSegDisk")
  i.vec <- seq_len(res$n)
  search_models(problem.dir, res$penalty[i.vec], res$iteration[i.vec], res$under[i.vec],
                res$over[i.vec], res$chosen)
}

parallelSearch_dir_batch <- function
### parallelSearch_dir on several problem directories in lockstep: every directory gets the
### result parallelSearch_dir(problem.dir, peaks.int, width) gives, and all models the searches
### ask for in a round are computed in one launch.  devices: "all" or GPU ids, the directories
### dealt to one shard per listed GPU.
(problem.dir.vec, peaks.int.vec, width=0L, verbose=0, devices=NULL){
  stopifnot(is.character(problem.dir.vec), is.integer(peaks.int.vec), all(0 <= peaks.int.vec))
  stopifnot(is.integer(width) && length(width)==1 && 0 <= width && width <= 256)
  n <- length(problem.dir.vec)
  saved <- set_devices_knob(devices)
  on.exit(restore_devices_knob(saved), add=TRUE)
  peaks.int.vec <- rep(peaks.int.vec, l=n)
  capacity <- 1024L
  res <- .C(
    "PeakSegFPOP_parallel_search_batch_interface",
    problem.dir.vec, as.integer(n), peaks.int.vec, width, as.integer(verbose), capacity,
    penalty=rep(strrep(" ", 39), capacity*n), iteration=integer(capacity*n),
    under=integer(capacity*n), over=integer(capacity*n),
    n.models=integer(n), chosen=integer(n), status=integer(n),
    PACKAGE="PeakSegDisk")
  if(any(res$status != 0)){
    stop("error code ", res$status[res$status != 0][1])
  }
  lapply(seq_len(n), function(d){
    i.vec <- (d-1L)*capacity + seq_len(res$n.models[d])
    search_models(problem.dir.vec[d], res$penalty[i.vec], res$iteration[i.vec], res$under[i.vec],
                  res$over[i.vec], res$chosen[d])
  })
}
