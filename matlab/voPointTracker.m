classdef voPointTracker < handle
%VOPOINTTRACKER libvo (MI355X) stand-in for vision.PointTracker: pyramidal Lucas-Kanade.
%   tracker = voPointTracker('NumPyramidLevels', 3, 'BlockSize', [31 31], ...
%                            'MaxIterations', 30, 'MaxBidirectionalError', inf);
%   initialize(tracker, points, I);
%   [points, validity, scores] = step(tracker, I);
%   setPoints(tracker, points);  setPoints(tracker, points, validity);  release(tracker);
%   points is M x 2 [x y], 1-based; I a uint8 grey image.  step carries every
%   valid point from the previous image to I on the device (vo_mex('trackpoints'))
%   and keeps I for the next step.  A point that is lost keeps its last
%   position and stays invalid until setPoints, as the toolbox's tracker does.
%   BlockSize is [height width], odd, 5 .. 31; NumPyramidLevels 1 .. 6;
%   MaxIterations 1 .. 50.  The arithmetic is the fixed-point algorithm written
%   down in DESIGN.md 3.5.3, not the toolbox's closed one: positions agree to
%   tracking accuracy, not by bits.  For stereo use the left image as the
%   previous and the right one as the next.
    properties
        NumPyramidLevels = 3
        BlockSize = [31 31]
        MaxIterations = 30
        MaxBidirectionalError = inf
    end
    properties (Access = private)
        Image = []
        Points = zeros(0, 2, 'single')
        Validity = false(0, 1)
    end
    methods
        function obj = voPointTracker(varargin)
            p = inputParser;
            p.addParameter('NumPyramidLevels', 3);
            p.addParameter('BlockSize', [31 31]);
            p.addParameter('MaxIterations', 30);
            p.addParameter('MaxBidirectionalError', inf);
            p.parse(varargin{:});
            obj.NumPyramidLevels = p.Results.NumPyramidLevels;
            obj.BlockSize = p.Results.BlockSize;
            obj.MaxIterations = p.Results.MaxIterations;
            obj.MaxBidirectionalError = p.Results.MaxBidirectionalError;
        end
        function initialize(obj, points, I)
            if ~isa(I, 'uint8') || ~ismatrix(I)
                error('vo:PointTracker:image', 'voPointTracker: I must be a uint8 grey image (im2gray, im2uint8)');
            end
            obj.Image = I;
            setPoints(obj, points);
        end
        function setPoints(obj, points, validity)
            if isobject(points), points = points.Location; end
            obj.Points = single(points);
            if nargin < 3, validity = true(size(obj.Points, 1), 1); end
            if numel(validity) ~= size(obj.Points, 1)
                error('vo:PointTracker:validity', 'voPointTracker: validity must have one entry per point');
            end
            obj.Validity = logical(validity(:));
        end
        function [points, validity, scores] = step(obj, I)
            if isempty(obj.Image)
                error('vo:PointTracker:notInitialized', 'voPointTracker: call initialize first');
            end
            opts = double([obj.NumPyramidLevels, obj.BlockSize(1), obj.BlockSize(2), obj.MaxIterations, obj.MaxBidirectionalError]);
            idx = find(obj.Validity);
            [p, ok, s] = vo_mex('trackpoints', obj.Image, I, obj.Points(idx, :), opts);
            scores = zeros(size(obj.Points, 1), 1, 'single');
            obj.Points(idx, :) = p;
            obj.Validity(idx) = ok;
            scores(idx) = s;
            obj.Image = I;
            points = obj.Points;
            validity = obj.Validity;
        end
        function release(obj)
            obj.Image = [];
            obj.Points = zeros(0, 2, 'single');
            obj.Validity = false(0, 1);
        end
    end
end
